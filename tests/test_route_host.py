"""``ProjectLayer.route`` - the one decision between a ``ProjectLayer`` call and its ``_lib`` call - without a GPU: every route
of the table in DESIGN.md §4.0a and every refusal, held to a table written out here (not derived by calling the function), on
CPU tensors; and the nets' front rule (``cuboid_proposal_net.front_rule``) against the decision over every layer-level case of
tests/route_cases.py: a spectrum it asks for is one ``get_voxel_zspectrum`` delivers, an ``out`` it hands is one ``get_voxel``
takes.  tests/test_gpu_route_census.py holds the launches themselves to the commit before the record."""
import types

import pytest
import torch

from selfpose3d_amd import _lib
from selfpose3d_amd.cuboid_proposal_net import Front, front_rule
from selfpose3d_amd.project_layer import Route
from tests import route_cases as rc

NHWC, PLANAR = _lib.LAYOUT_NHWC, _lib.LAYOUT_PLANAR
F32, BF16 = torch.float32, torch.bfloat16


def case(J=15, hand="planar", grad="no_grad", mode="auto", io="fp32", sw=(), hm=None):
    return dict(J=J, hand=hand, grad=grad, mode=mode, io=io, sw=tuple(sw), call="plain", hm=hm)


def decide(c, SZ=None, **kw):
    layer = rc.build_layer(c)
    hms, _ = rc.build_maps(c, "cpu")
    with rc.grad_context(c):
        return layer.route(hms, SZ, **kw)


def R(read, layout, jp, elem, write, J, cl=False, out=False, backward="none", autograd=False, widen=False):
    return Route(read, layout, jp, elem, write, J, cl, out, backward, autograd, widen)


G = "required"
# (what it is, the case, arguments of route(), the record) - one row per line of the table in DESIGN.md §4.0a, and the
# demotions and hand-overs around each
ROUTES = [
    # cubes, planar path
    ("planar: 33 joints", case(J=33), {}, R("planar", PLANAR, 0, F32, "cubes", 33, autograd=True)),
    ("planar: mode", case(mode="planar", grad=G), {}, R("planar", PLANAR, 0, F32, "cubes", 15, backward="planar", autograd=True)),
    ("planar: 17 joints with a gradient", case(J=17, grad=G), {}, R("planar", PLANAR, 0, F32, "cubes", 17, backward="planar", autograd=True)),
    ("planar: a one-pixel map", case(hm="24x1"), {}, R("planar", PLANAR, 0, F32, "cubes", 15, autograd=True)),
    ("planar: pad_channels and channels_last are dropped", case(mode="planar"), dict(pad_channels=True, channels_last=True),
     R("planar", PLANAR, 0, F32, "cubes", 15, autograd=True)),
    ("planar: bf16_maps changes nothing for fp32 maps", case(J=33, sw=["bf16_maps"]), {}, R("planar", PLANAR, 0, F32, "cubes", 33, autograd=True)),
    ("planar: bf16_maps widens bf16 maps", case(hand="nhwc_bf16", mode="planar", sw=["bf16_maps"]), {}, R("planar", PLANAR, 0, F32, "cubes", 15, autograd=True, widen=True)),
    # cubes, packed
    ("packed", case(), {}, R("packed", NHWC, 16, F32, "cubes", 15, autograd=True)),
    ("packed: grad enabled, none wanted", case(grad="enabled"), {}, R("packed", NHWC, 16, F32, "cubes", 15, autograd=True)),
    ("packed: 4 joints", case(J=4), {}, R("packed", NHWC, 4, F32, "cubes", 4, autograd=True)),
    ("packed: pad_channels", case(J=13), dict(pad_channels=True), R("packed", NHWC, 16, F32, "cubes", 16, autograd=True)),
    ("packed: channels_last needs J % 4 == 0 or the pad", case(J=13), dict(channels_last=True), R("packed", NHWC, 16, F32, "cubes", 13, autograd=True)),
    ("packed: channels_last", case(J=12), dict(channels_last=True), R("packed", NHWC, 12, F32, "cubes", 12, cl=True, autograd=True)),
    ("packed: pad + channels_last", case(J=13), dict(pad_channels=True, channels_last=True), R("packed", NHWC, 16, F32, "cubes", 16, cl=True, autograd=True)),
    ("packed: 17 joints drop pad + channels_last", case(J=17), dict(pad_channels=True, channels_last=True), R("packed", NHWC, 32, F32, "cubes", 17, autograd=True)),
    ("packed: out", case(hand="nhwc"), dict(want_grids=False, out=True), R("packed", NHWC, 16, F32, "cubes", 15, out=True, autograd=True)),
    ("packed: float64 maps", case(hand="f64"), {}, R("packed", NHWC, 16, F32, "cubes", 15, autograd=True)),
    ("packed: bf16 storage", case(io="bf16", hand="nhwc_bf16"), {}, R("packed", NHWC, 16, BF16, "cubes", 15, autograd=True)),
    ("packed: bf16 storage, 32 joints", case(J=32, io="bf16"), {}, R("packed", NHWC, 32, BF16, "cubes", 32, autograd=True)),
    ("packed: one joint, the switch off", case(J=1, hand="slice_planar"), {}, R("packed", NHWC, 4, F32, "cubes", 1, autograd=True)),
    ("packed: one joint that does not classify", case(J=1, hand="expanded", sw=["one_channel"]), {}, R("packed", NHWC, 4, F32, "cubes", 1, autograd=True)),
    ("packed, 16-bit mask", case(grad=G), {}, R("packed", NHWC, 16, F32, "cubes", 15, backward="mask16", autograd=True)),
    ("packed, 16-bit mask: one joint under one_channel", case(J=1, hand="slice_planar", grad=G, sw=["one_channel"]), dict(pad_channels=True),
     R("packed", NHWC, 4, F32, "cubes", 4, backward="mask16", autograd=True)),
    ("packed, two-plane mask", case(J=17, grad=G, sw=["wide_grad"]), {}, R("packed", NHWC, 32, F32, "cubes", 17, backward="mask2x16", autograd=True)),
    ("packed, two-plane mask: mode nhwc", case(J=32, grad=G, mode="nhwc", sw=["wide_grad"]), {}, R("packed", NHWC, 32, F32, "cubes", 32, backward="mask2x16", autograd=True)),
    ("packed, planar backward: bf16 storage", case(io="bf16", grad=G), {}, R("packed", NHWC, 16, BF16, "cubes", 15, backward="planar", autograd=True)),
    ("packed, planar backward: a one-pixel map under mode nhwc", case(mode="nhwc", grad=G, hm="24x1"), {},
     R("packed", NHWC, 16, F32, "cubes", 15, backward="planar", autograd=True)),
    ("packed: wide_grad is an fp32 switch", case(J=17, io="bf16", sw=["wide_grad"]), {}, R("packed", NHWC, 32, BF16, "cubes", 17, autograd=True)),
    # cubes, one channel in place
    ("one: slice of a planar tensor", case(J=1, hand="slice_planar", sw=["one_channel"]), {}, R("one", PLANAR, 15, F32, "cubes", 1, autograd=True)),
    ("one: slice of nhwc views, padded, into out", case(J=1, hand="slice_nhwc", sw=["one_channel"]), dict(want_grids=False, out=True),
     R("one", NHWC, 16, F32, "cubes", 1, out=True, autograd=True)),
    ("one: pad + channels_last", case(J=1, hand="contiguous1", mode="nhwc", sw=["one_channel"]), dict(pad_channels=True, channels_last=True),
     R("one", PLANAR, 1, F32, "cubes", 4, cl=True, autograd=True)),
    ("one, training pair", case(J=1, hand="slice_nhwc", grad=G, sw=["one_channel_grad"]), dict(pad_channels=True),
     R("one", NHWC, 16, F32, "cubes", 4, backward="one", autograd=True)),
    ("one, training pair: not without a gradient", case(J=1, hand="slice_nhwc", sw=["one_channel_grad"]), {}, R("packed", NHWC, 4, F32, "cubes", 1, autograd=True)),
    # cubes, bf16_maps
    ("bf16 maps, packed", case(hand="nhwc_bf16", sw=["bf16_maps"]), dict(pad_channels=True, channels_last=True),
     R("packed", NHWC, 16, BF16, "cubes", 16, cl=True)),
    ("bf16 maps, packed: fp32 producer, 17 joints, out", case(J=17, sw=["bf16_maps"]), dict(want_grids=False, out=True),
     R("packed", NHWC, 32, BF16, "cubes", 17, out=True)),
    ("bf16 maps: a gradient ignores the switch", case(hand="nhwc_bf16", grad=G, sw=["bf16_maps"]), {}, R("packed", NHWC, 16, F32, "cubes", 15, backward="mask16", autograd=True)),
    ("bf16 maps: 12 joints widen", case(J=12, hand="nhwc_bf16", sw=["bf16_maps"]), {}, R("packed", NHWC, 12, F32, "cubes", 12, autograd=True, widen=True)),
    ("bf16 maps: fp32 tensors of one joint keep the fp32 one-channel route", case(J=1, hand="slice_nhwc", sw=["bf16_maps", "one_channel"]), {},
     R("one", NHWC, 16, F32, "cubes", 1, autograd=True)),
    ("bf16 maps: 12 joints of an fp32 producer have nothing to widen", case(J=12, sw=["bf16_maps"]), {}, R("packed", NHWC, 12, F32, "cubes", 12, autograd=True)),
    # z-spectrum
    ("zdft", case(J=13), dict(SZ=28), R("packed", NHWC, 16, F32, "zdft", 13)),
    ("zspectrum: 17 joints", case(J=17, sw=["wide_zspectrum"]), dict(SZ=28), R("packed", NHWC, 32, F32, "zspectrum", 17)),
    ("zspectrum: bf16 maps", case(J=16, mode="nhwc", sw=["bf16_maps"]), dict(SZ=28), R("packed", NHWC, 16, BF16, "zspectrum", 16)),
    ("zspectrum: bf16 maps, 32 joints", case(J=32, sw=["bf16_maps", "wide_zspectrum"]), dict(SZ=28), R("packed", NHWC, 32, BF16, "zspectrum", 32)),
    ("one_zspectrum", case(J=1, hand="slice_planar", sw=["one_zspectrum"]), dict(SZ=28), R("one", PLANAR, 15, F32, "one_zspectrum", 1)),
    ("one_zspectrum: fp32 maps under bf16_maps", case(J=1, hand="slice_nhwc", sw=["one_zspectrum", "bf16_maps"]), dict(SZ=28),
     R("one", NHWC, 16, F32, "one_zspectrum", 1)),
]


@pytest.mark.parametrize("what,c,kw,want", ROUTES, ids=[r[0] for r in ROUTES])
def test_route_table(what, c, kw, want):
    got = decide(c, kw.pop("SZ", None), **kw)
    assert got == want and isinstance(got, Route)


def _bf16_slice(hand):
    """a bf16 one-channel list: a slice of bf16 nhwc views / of a planar bf16 tensor / an expanded bf16 tensor"""
    from selfpose3d_amd.project_layer import nhwc_heatmap_views
    w, h = rc.HM
    if hand == "nhwc":
        return [x[:, 2:3] for x in nhwc_heatmap_views(torch.zeros(rc.V, rc.B, h, w, 16, dtype=BF16), 15)]
    if hand == "planar":
        return [torch.zeros(rc.B, 15, h, w, dtype=BF16)[:, 2:3] for _ in range(rc.V)]
    return [torch.zeros(1, 1, h, w, dtype=BF16).expand(rc.B, 1, h, w) for _ in range(rc.V)]


def test_bf16_one_channel_routes():
    """bf16 tensors under ``bf16_maps``: read in place where they classify (2-byte elements); an expanded one does not, is
    widened - and the widened tensor is dense, which the fp32 one-channel route reads as a planar (B,1,h,w)"""
    layer = rc.build_layer(case(sw=["bf16_maps", "one_channel", "one_zspectrum"]))
    with torch.no_grad():
        assert layer.route(_bf16_slice("nhwc")) == R("one", NHWC, 16, BF16, "cubes", 1)
        assert layer.route(_bf16_slice("planar"), pad_channels=True) == R("one", PLANAR, 15, BF16, "cubes", 4)
        assert layer.route(_bf16_slice("expanded")) == R("one", PLANAR, 1, F32, "cubes", 1, autograd=True, widen=True)
        assert layer.route(_bf16_slice("nhwc"), 28) == R("one", NHWC, 16, BF16, "one_zspectrum", 1)
        layer.one_channel = False
        assert layer.route(_bf16_slice("nhwc")) == R("packed", NHWC, 4, F32, "cubes", 1, autograd=True, widen=True)
        layer.bf16_maps = False      # bf16 tensors without the switch: the classifier answers for fp32 elements, cubes are re-tiled
        assert layer.spectrum_route(_bf16_slice("nhwc")) is None
        assert layer.route(_bf16_slice("nhwc")) == R("packed", NHWC, 4, F32, "cubes", 1, autograd=True)


NHWC_GRAD = "differentiates at most 16 joints"
STORAGE = "bf16 storage needs the NHWC path with 13..32 joints"
OUT = r"get_voxel\(out=...\): planar NHWC-path result without grids only"
EXCLUDE = "exclude each other"
SPECTRUM = "get_voxel_zspectrum: fp32 NHWC path with 13..16 joints only"
REFUSALS = [
    ("mode nhwc, 17 joints, gradient", case(J=17, mode="nhwc", grad=G), {}, NHWC_GRAD),
    ("mode nhwc, 33 joints, gradient", case(J=33, mode="nhwc", grad=G, sw=["wide_grad"]), {}, NHWC_GRAD),
    ("mode nhwc, 17 joints, gradient, wide_grad with bf16 storage", case(J=17, mode="nhwc", grad=G, io="bf16", sw=["wide_grad"]), {}, NHWC_GRAD),
    ("bf16 storage, 12 joints", case(J=12, io="bf16"), {}, STORAGE),
    ("bf16 storage, planar mode", case(io="bf16", mode="planar"), {}, STORAGE),
    ("bf16 storage, 33 joints", case(J=33, io="bf16", mode="nhwc"), {}, STORAGE),
    ("bf16 storage before the out refusal", case(J=12, io="bf16"), dict(out=True), STORAGE),
    ("out on the planar path", case(mode="planar"), dict(want_grids=False, out=True), OUT),
    ("out under a one-pixel map", case(hm="24x1"), dict(want_grids=False, out=True), OUT),
    ("out with grids", case(), dict(out=True), OUT),
    ("out with pad_channels", case(), dict(want_grids=False, pad_channels=True, out=True), OUT),
    ("out with channels_last", case(J=16), dict(want_grids=False, channels_last=True, out=True), OUT),
    ("out with a masked gradient", case(grad=G), dict(want_grids=False, out=True), OUT),
    ("out with the one-channel training pair", case(J=1, hand="slice_planar", grad=G, sw=["one_channel_grad"]), dict(want_grids=False, out=True), OUT),
    ("bf16_maps with bf16 storage", case(io="bf16", sw=["bf16_maps"]), {}, EXCLUDE),
    ("bf16_maps with bf16 storage, gradient", case(io="bf16", grad=G, sw=["bf16_maps"]), {}, EXCLUDE),
    ("bf16_maps with bf16 storage, spectrum", case(io="bf16", sw=["bf16_maps"]), dict(SZ=28), EXCLUDE),
    ("spectrum: 12 joints", case(J=12), dict(SZ=28), SPECTRUM),
    ("spectrum: 17 joints, the switch off", case(J=17), dict(SZ=28), SPECTRUM),
    ("spectrum: 33 joints", case(J=33, sw=["wide_zspectrum"]), dict(SZ=28), SPECTRUM),
    ("spectrum: one joint, the switch off", case(J=1, hand="slice_planar"), dict(SZ=28), SPECTRUM),
    ("spectrum: one joint that does not classify", case(J=1, hand="expanded", sw=["one_zspectrum"]), dict(SZ=28), SPECTRUM),
    ("spectrum: planar mode", case(mode="planar"), dict(SZ=28), SPECTRUM),
    ("spectrum: bf16 storage", case(io="bf16"), dict(SZ=28), SPECTRUM),
    ("spectrum: a one-pixel map", case(hm="24x1"), dict(SZ=28), SPECTRUM),
]


@pytest.mark.parametrize("what,c,kw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, c, kw, message):
    with pytest.raises(_lib.Sp3dError, match=message):
        decide(c, kw.pop("SZ", None), **kw)


class _Cuda:
    """stands where a GPU heat-map would (tests/test_one_front_host.py): everything the decision reads, answered by a CPU tensor"""
    is_cuda = True

    def __init__(self, t):
        self.t, self.shape, self.dtype, self.device, self.requires_grad = t, t.shape, t.dtype, t.device, t.requires_grad

    def dim(self):
        return self.t.dim()

    def stride(self):
        return self.t.stride()


ARGS = ([], list(rc.SPACE), [list(rc.CENTER)], list(rc.CUBE))


def test_launcher_refusals_before_the_route():
    """what the launchers refuse themselves, in front of the decision: a gradient through the spectrum, CPU tensors, a
    heat-map of another size than the config's"""
    layer = rc.build_layer(case())
    hms, _ = rc.build_maps(case(grad=G), "cpu")
    with torch.enable_grad(), pytest.raises(_lib.Sp3dError, match="is an inference path"):
        layer.get_voxel_zspectrum([_Cuda(x) for x in hms], *ARGS, 28)
    with torch.no_grad():
        for call in (lambda m: layer.get_voxel(m, *ARGS), lambda m: layer.get_voxel_zspectrum(m, *ARGS, 28)):
            with pytest.raises(_lib.Sp3dError, match="must be on the GPU"):
                call(hms)
            with pytest.raises(_lib.Sp3dError, match=r"heat-map tensor is 24x1 but cfg.NETWORK.HEATMAP_SIZE is \[24, 18\]"):
                call([_Cuda(x) for x in rc.build_maps(case(hm="24x1"), "cpu")[0]])
            with pytest.raises(_lib.Sp3dError, match=EXCLUDE):          # the route's refusals come after these two
                rc.build_layer(case(io="bf16", sw=["bf16_maps"])).get_voxel([_Cuda(x) for x in hms], *ARGS)


class _V2V:
    """a V2V net that wants whatever the layer can give: FFT opening conv, the spectrum of any channel count"""

    def __init__(self, cl16):
        self.cl16 = cl16

    def wants_planar_input(self):
        return True

    def wants_zspectrum(self, X, Y, Z, cin):
        return rc.SZ

    def wants_channels_last_cubes(self, X, Y, Z):
        return self.cl16


@pytest.mark.parametrize("fronts", [(), ("one",), ("zdft", "wide", "one")])
def test_front_rule_and_decision_cannot_disagree(fronts):
    """over every layer-level case of the census: a spectrum the rule asks for is one the decision delivers, an ``out`` it hands
    is one the decision takes, and a front the caller did not name is not taken"""
    seen = {"sz": 0, "out": 0, "plain": 0}
    for c in rc.layer_cases():
        layer = rc.build_layer(c)
        hms = [_Cuda(x) for x in rc.build_maps(c, "cpu")[0]]
        for cl16 in (False, True):
            net = types.SimpleNamespace(project_layer=layer, v2v_net=_V2V(cl16), cube_size=list(rc.CUBE), channels_last=True,
                                        rootnet_roothm=True)
            with rc.grad_context(c):
                front = front_rule(net, hms, fronts)
                assert isinstance(front, Front)
                if front.sz is not None:
                    route = layer.route(hms, front.sz)              # does not raise
                    kind = "one" if route.read == "one" else ("wide" if route.jp == 32 else "zdft")
                    assert kind in fronts and not front.out, rc.case_id(c)
                    seen["sz"] += 1
                elif front.out:
                    route = layer.route(hms, None, False, front.pad_channels, front.channels_last, True)
                    assert route.out and not (front.pad_channels or front.channels_last), rc.case_id(c)
                    seen["out"] += 1
                else:
                    seen["plain"] += 1
    assert seen["out"] > 50 and seen["plain"] > 50 and (seen["sz"] > 20 or not fronts), seen
