"""Which ``_lib`` calls a ``ProjectLayer`` call, a root net and the pose net make: the cases, and the recording run.

tools/record_route_census.py runs every case against the commit BEFORE the typed route record existed and writes
tests/golden/route_census.json; tests/test_gpu_route_census.py replays them on the current tree and compares;
tests/test_route_host.py classifies the layer-level ones on CPU tensors.  Only names that commit already had are used here.

Layer level: heat-maps 24 x 18, image 96 x 72, V = 3, B = 2, cube (8, 12, 20), SZ = 28, space (8000, 8000, 2000) - the smallest
geometry every route accepts.  The axes are covered pairwise (every value of one axis meets every value of every other axis
in some case, where the pair exists at all), not as the full product; the one-pixel map and the capture context are
explicit lists.  Net level: the setup of tests/test_gpu_one_front.py::_root_setup (24 x 18 maps, cube 80 x 80 x 20, B = 2,
V = 5) for three root nets, and the pose net on 16^3 person cubes (the smallest cube the suite runs the V2V inference plan
at); the V2V stack itself is replaced by a stub that records what it is handed - the routes end where it begins."""
import contextlib
import inspect
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG, HM = (96, 72), (24, 18)                       # (w, h)
V, B, P = 3, 2, 3
CUBE, SZ, SPACE = (8, 12, 20), 28, (8000.0, 8000.0, 2000.0)
CENTER = (0.0, -500.0, 800.0)

JOINTS = (1, 4, 12, 13, 15, 16, 17, 32, 33)
HAND_OVERS = ("planar", "f64", "nhwc", "nhwc_bf16", "slice_planar", "slice_nhwc", "contiguous1", "expanded")
ONE_ONLY = HAND_OVERS[4:]                          # a list[V] of (B,1,h,w): J = 1
GRADS = ("no_grad", "enabled", "required")
MODES = ("auto", "nhwc", "planar")
STORAGE = ("fp32", "bf16")
SWITCH_NAMES = ("one_channel", "one_channel_grad", "wide_grad", "wide_zspectrum", "one_zspectrum", "bf16_maps")
SWITCHES = ((),) + tuple((s,) for s in SWITCH_NAMES) + \
    (("bf16_maps", "one_channel"), ("bf16_maps", "wide_zspectrum"), ("bf16_maps", "one_zspectrum"))
CALLS = ("plain", "no_grids", "pad", "cl", "pad_cl", "sample_of", "out", "zspectrum")
AXES = (("J", JOINTS), ("hand", HAND_OVERS), ("grad", GRADS), ("mode", MODES), ("io", STORAGE), ("sw", SWITCHES), ("call", CALLS))

LIB_NAMES = ("unproject_fwd", "pack_heatmaps", "unproject_fwd_zdft", "unproject_fwd_zspectrum", "unproject_one_fwd_zspectrum",
             "unproject_one_fwd_train", "unproject_bwd", "unproject_bwd_packed", "unproject_one_bwd")


def _exists(J, hand):
    if hand in ONE_ONLY:
        return J == 1
    return J <= 32 or hand in ("planar", "f64")    # nhwc_heatmap_views: a pixel holds at most 32 channels


BASE = dict(J=15, hand="planar", grad="no_grad", mode="auto", io="fp32", sw=(), call="plain")


def case_id(c):
    """the axes on which a case leaves BASE, e.g. ``J1,slice_nhwc,required,one_channel_grad,pad_cl``"""
    show = dict(J="J%d", hand="%s", grad="%s", mode="mode=%s", io="io=%s", call="%s")
    parts = [show[k] % c[k] if k != "sw" else "+".join(c[k]) for k in BASE if c[k] != BASE[k]]
    return ",".join(parts + [c[k] for k in ("hm", "ctx") if c.get(k)]) or "base"


def _pairwise():
    """greedy pairwise cover of AXES, the same list on every run (a congruential generator of its own, no library RNG)"""
    state = [12345]

    def rnd(n):
        state[0] = (state[0] * 1103515245 + 12345) & 0x7fffffff
        return (state[0] >> 8) % n

    names = [a for a, _ in AXES]
    todo = set()
    for i, (a, va) in enumerate(AXES):
        for b, vb in AXES[i + 1:]:
            for x in va:
                for y in vb:
                    if {a, b} != {"J", "hand"} or _exists(*((x, y) if a == "J" else (y, x))):
                        todo.add((a, x, b, y))

    def pairs(c):
        return {(a, c[a], b, c[b]) for i, a in enumerate(names) for b in names[i + 1:]}

    out = []
    while todo:
        best, gain = None, -1
        for _ in range(300):
            c = {a: vals[rnd(len(vals))] for a, vals in AXES}
            if not _exists(c["J"], c["hand"]):
                continue
            g = len(pairs(c) & todo)
            if g > gain:
                best, gain = c, g
        if gain <= 0:                              # the sampler missed the last pairs: build a case around one of them
            a, x, b, y = sorted(todo, key=repr)[0]
            best = {n: vals[0] for n, vals in AXES}
            best.update({a: x, b: y})
            if not _exists(best["J"], best["hand"]):
                best["J" if "hand" in (a, b) else "hand"] = 1 if "hand" in (a, b) else "planar"
        todo -= pairs(best)
        out.append(best)
    return out


def layer_cases():
    seen, out = set(), []

    def add(**kw):
        c = dict(BASE, **kw)
        if _exists(c["J"], c["hand"]) and case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)

    add()
    for c in _pairwise():
        add(**c)
    # every switch (and pair) at the joint counts and hand-overs it is about, without and with a wanted gradient
    about = {"one_channel": ((1, "slice_planar"), (1, "slice_nhwc")), "one_channel_grad": ((1, "slice_planar"), (1, "slice_nhwc")),
             "wide_grad": ((17, "planar"), (17, "nhwc")), "wide_zspectrum": ((17, "planar"), (17, "nhwc")),
             "one_zspectrum": ((1, "slice_planar"), (1, "slice_nhwc")), "bf16_maps": ((15, "nhwc_bf16"), (17, "planar"), (12, "nhwc_bf16"))}
    for sw in SWITCHES[1:]:
        for J, hand in about[sw[-1]] + (((1, "slice_nhwc"),) if sw == ("bf16_maps", "one_channel") else ()):
            add(J=J, hand=hand, call="pad_cl", sw=sw)
            add(J=J, hand=hand, call="pad_cl", sw=sw, grad="required")
            add(J=J, hand=hand, call="out", sw=sw)
            add(J=J, hand=hand, call="zspectrum", sw=sw)
    # one heat-map of 24 x 1, below 2 x 2
    for mode in ("auto", "nhwc"):
        for call in ("plain", "out", "zspectrum"):
            add(mode=mode, call=call, hm="24x1")
        add(mode=mode, grad="required", hm="24x1")
    add(call="out", sw=("bf16_maps",), hm="24x1")
    # inside static_camera_table(...) the call is made twice on the same maps: the pack cache is off, every call re-tiles
    for J, hand, sw in ((15, "planar", ()), (15, "nhwc", ()), (15, "f64", ()), (1, "slice_planar", ("one_channel",)),
                        (15, "planar", ("bf16_maps",)), (17, "planar", ("wide_zspectrum",))):
        for call in ("no_grids", "zspectrum"):
            add(J=J, hand=hand, sw=sw, call=call, ctx="capture")
    add(ctx="twice")                                   # ... and outside it the second call is served from the cache
    add(grad="required", ctx="capture")
    return out


# ---- building the inputs of a layer-level case ------------------------------------------------------------------------------
def hm_size(c):
    return (24, 1) if c.get("hm") == "24x1" else HM


def build_maps(c, device):
    """the heat-map list of a case -> (list[V] of (B,J,h,w), the tensors a gradient is asked of)"""
    from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views
    w, h = hm_size(c)
    J, hand, grad = c["J"], c["hand"], c["grad"] == "required"
    g = torch.Generator().manual_seed(7)
    rand = lambda *s: torch.rand(*s, generator=g).to(device)
    if hand in ("planar", "f64", "contiguous1"):
        leaves = [rand(B, J, h, w).to(torch.float64 if hand == "f64" else torch.float32).requires_grad_(grad) for _ in range(V)]
        return leaves, leaves
    if hand == "expanded":
        leaves = [rand(1, 1, h, w).requires_grad_(grad) for _ in range(V)]
        return [x.expand(B, 1, h, w) for x in leaves], leaves
    if hand == "slice_planar":
        leaves = [rand(B, 15, h, w).requires_grad_(grad) for _ in range(V)]
        return [x[:, 2:3] for x in leaves], leaves
    Jn = 15 if hand == "slice_nhwc" else J
    jp = ProjectLayer.jp_for(Jn)
    buf = rand(V, B, h, w, jp)
    buf[..., Jn:] = 0
    buf = buf.to(torch.bfloat16 if hand == "nhwc_bf16" else torch.float32).requires_grad_(grad)
    views = nhwc_heatmap_views(buf, Jn)
    return ([x[:, 2:3] for x in views] if hand == "slice_nhwc" else views), [buf]


def build_layer(c):
    from selfpose3d_amd.config import load_config
    from selfpose3d_amd.project_layer import ProjectLayer
    cfg = load_config(None, NETWORK__IMAGE_SIZE=list(IMG), NETWORK__HEATMAP_SIZE=list(hm_size(c)))
    layer = ProjectLayer(cfg, mode=c["mode"], io_dtype=torch.bfloat16 if c["io"] == "bf16" else torch.float32)
    for s in SWITCH_NAMES:
        setattr(layer, s, s in c["sw"])
    layer.deterministic_backward = False
    return layer


def grad_context(c):
    return torch.no_grad() if c["grad"] == "no_grad" else torch.enable_grad()


def call_kwargs(c, device):
    """(grid_center, keyword arguments of get_voxel) of a case's call form; ``out`` is a view of a padded buffer"""
    X, Y, Z = CUBE
    call = c["call"]
    kw = dict(want_grids=call not in ("no_grids", "out", "pad_cl"), pad_channels=call in ("pad", "pad_cl"),
              channels_last=call in ("cl", "pad_cl"))
    centre = [list(CENTER)]
    if call == "sample_of":
        kw["sample_of"] = torch.tensor([0, 1, 1], device=device)
        centre = torch.tensor([CENTER] * P, device=device)
    if call == "out":
        dt = torch.bfloat16 if c["io"] == "bf16" else torch.float32
        kw["out"] = torch.zeros((B, c["J"], X + 2, Y + 4, Z + 8), dtype=dt, device=device)[:, :, :X, :Y, :Z]
    return centre, kw


# ---- recording ------------------------------------------------------------------------------------------------------------
def _tensor(t):
    """[dtype, shape, strides, requires_grad]"""
    return [str(t.dtype)[6:], list(t.shape), list(t.stride()), bool(t.requires_grad)]


class Recorder:
    """wrappers around the ``_lib`` entry points of LIB_NAMES and around ``ProjectLayer.get_voxel`` / ``get_voxel_zspectrum``
    that write down how they are called and call through.  Per call only what the route decides is kept: the geometry
    (map size, cube, number of views) is the case's own and would repeat in every line"""

    def __init__(self, layer_calls=True):
        self.calls, self.producers, self.layer_calls = [], set(), layer_calls

    def produced(self, tensors):
        self.producers = {t.untyped_storage().data_ptr() for t in tensors}

    FLAGS = ("want_grids", "pad_channels", "channels_last", "wide_mask", "one_channel", "wide", "deterministic")

    def _lib_entry(self, name, args):
        """numbers as passed; of the flags, ``out`` and ``sample_of`` only the ones that are set"""
        d = dict(fn=name)
        d.update({k: int(args[k]) for k in ("layout", "jp", "J", "B", "batch", "SZ") if k in args})
        views = args.get("views", args.get("hms"))
        if views is not None:           # element type the kernel is handed, and whether it reads the producer's own memory
            d["views"] = [str(views[0].dtype)[6:], views[0].untyped_storage().data_ptr() in self.producers]
        on = [k for k in self.FLAGS if args.get(k)] + [k for k in ("out", "sample_of") if args.get(k) is not None]
        if on:
            d["set"] = on
        if args.get("out_dtype") not in (None, torch.float32):
            d["out_dtype"] = str(args["out_dtype"])[6:]
        if args.get("pass_mask") is not None:
            d["pass_mask"] = list(args["pass_mask"].shape)
        if "grad_cubes" in args:
            d["grad_cubes"] = str(args["grad_cubes"].dtype)[6:]
        self.calls.append(d)

    def _layer_entry(self, name, args):
        if not self.layer_calls:
            return
        hms = args["heatmaps"]
        d = dict(fn=name, maps=[str(hms[0].dtype)[6:], int(hms[0].shape[1])])
        on = [k for k in self.FLAGS if args.get(k)] + [k for k in ("out", "sample_of") if args.get(k) is not None]
        if on:
            d["set"] = on
        if "SZ" in args:
            d["SZ"] = int(args["SZ"])
        self.calls.append(d)

    @contextlib.contextmanager
    def installed(self):
        from selfpose3d_amd import _lib
        from selfpose3d_amd.project_layer import ProjectLayer
        saved = []

        def wrap(owner, name, note):
            inner = getattr(owner, name)
            sig = inspect.signature(inner)

            def outer(*a, **k):
                bound = sig.bind(*a, **k)
                bound.apply_defaults()
                note(name, bound.arguments)
                return inner(*a, **k)
            saved.append((owner, name, inner))
            setattr(owner, name, outer)

        for name in LIB_NAMES:
            wrap(_lib, name, self._lib_entry)
        for name in ("get_voxel", "get_voxel_zspectrum"):
            wrap(ProjectLayer, name, self._layer_entry)
        try:
            yield self
        finally:
            for owner, name, inner in saved:
                setattr(owner, name, inner)


def _outcome(rec, fn):
    """run ``fn`` under the recorder -> ("raises", message) or dict(calls, result)"""
    from selfpose3d_amd import _lib
    rec.calls = []
    try:
        with rec.installed():
            result = fn()
    except _lib.Sp3dError as e:
        return ["raises", str(e)]
    except (AssertionError, TypeError) as e:       # what is no refusal of the layer's is told apart by its type
        return ["raises", type(e).__name__ + ": " + str(e).split("\n")[0]]
    return dict(calls=rec.calls, result=result)


def run_layer_case(c, device):
    from selfpose3d_amd import synthetic as syn
    from selfpose3d_amd.project_layer import clear_pack_cache
    clear_pack_cache()
    rec = Recorder(layer_calls=False)       # the layer-level call is the case itself
    layer = build_layer(c)
    hms, leaves = build_maps(c, device)
    rec.produced(hms)
    meta = syn.make_meta(B, V, list(IMG))
    centre, kw = call_kwargs(c, device)
    repeats = 2 if c.get("ctx") else 1

    def once():
        if c["call"] == "zspectrum":
            return [_tensor(layer.get_voxel_zspectrum(hms, meta, list(SPACE), centre, list(CUBE), SZ))]
        cubes, grids = layer.get_voxel(hms, meta, list(SPACE), centre, list(CUBE), **kw)
        out = [_tensor(cubes), None if grids is None else _tensor(grids)]
        if kw.get("out") is not None:
            out.append(cubes.data_ptr() == kw["out"].data_ptr())
        if c["grad"] == "required" and cubes.requires_grad:
            cubes.sum().backward()
            out.append([None if x.grad is None else [str(x.grad.dtype), list(x.grad.shape)] for x in leaves])
        return out

    def run():
        with grad_context(c):
            if c.get("ctx") == "capture":
                table = layer.camera_table(meta, B, None, device)
                with layer.static_camera_table(table):
                    return [once() for _ in range(repeats)]
            return [once() for _ in range(repeats)]

    got = _outcome(rec, run)
    clear_pack_cache()
    return got


# ---- net level --------------------------------------------------------------------------------------------------------------
NET_CONFIGS = {          # name -> (yaml, overrides): the one-channel root net, the 15-joint root net, the 17-joint root net
    "roothm": ("cam5_posenet.yaml", {}),
    "joints15": ("cam5_posenet.yaml", dict(NETWORK__ROOTNET_ROOTHM=False)),
    "coco17": ("shelf_synthetic_coco17_cam5.yaml", {}),
}
NET_FRONTS = {"roothm": "one", "joints15": "zdft", "coco17": "wide"}
NET_B, NET_V = 2, 5
POSE_CUBE = [16, 16, 16]     # the person cube of the pose-net cases


def net_cases():
    out = []
    for cfg in NET_CONFIGS:
        for net in ("plain", "soft"):
            for hand in ("planar", "nhwc", "nhwc_bf16"):
                for front in (False, True):
                    for grad in (False, True):
                        out.append(dict(kind="root", cfg=cfg, net=net, hand=hand, front=front, grad=grad, bf16_maps=False))
                if hand == "nhwc_bf16":
                    for front in (False, True):
                        out.append(dict(kind="root", cfg=cfg, net=net, hand=hand, front=front, grad=False, bf16_maps=True))
        out.append(dict(kind="root", cfg=cfg, net="plain", hand="nhwc", front=True, grad=False, bf16_maps=False, one_channel=True))
        out.append(dict(kind="train_rootnet", cfg=cfg))
    for mode in ("auto", "planar"):      # with and without the direct hand-over of the person cubes
        out.append(dict(kind="pose", cfg="joints15", mode=mode, cube=POSE_CUBE))
    return out


def net_case_id(c):
    if c["kind"] == "root":
        return "{cfg},{net},{hand},front{front:d},grad{grad:d}".format(**c) + "".join("," + k for k in ("bf16_maps", "one_channel") if c.get(k))
    if c["kind"] == "train_rootnet":
        return c["cfg"] + ",train_rootnet"
    return "pose,mode={mode},cube{0}".format(c["cube"][0], **c)


_nets = {}


def _net_setup(name, device):
    if (name, str(device)) not in _nets:
        from selfpose3d_amd import _lib, synthetic as syn
        from selfpose3d_amd.config import load_config
        from selfpose3d_amd.cuboid_proposal_net import CuboidProposalNet
        from selfpose3d_amd.cuboid_proposal_net_soft import CuboidProposalNetSoft
        from selfpose3d_amd.pose_regression_net import PoseRegressionNet
        from selfpose3d_amd.project_layer import ProjectLayer, nhwc_heatmap_views
        yaml, over = NET_CONFIGS[name]
        cfg = load_config(os.path.join(ROOT, "configs", yaml), NETWORK__IMAGE_SIZE=list(IMG), NETWORK__HEATMAP_SIZE=list(HM),
                          PICT_STRUCT__CUBE_SIZE=list(POSE_CUBE), **over)
        assert [int(v) for v in cfg.MULTI_PERSON.INITIAL_CUBE_SIZE] == [80, 80, 20]
        J = int(cfg.NETWORK.NUM_JOINTS)
        nets = dict(plain=CuboidProposalNet(cfg), soft=CuboidProposalNetSoft(cfg), pose=PoseRegressionNet(cfg))
        for n in nets.values():
            n.to(device).eval().use_channels_last(True)
        planar = [h.to(device) for h in syn.random_heatmaps(NET_B, NET_V, J, HM[1], HM[0], seed=41)]
        jp = ProjectLayer.jp_for(J)
        packed = _lib.pack_heatmaps(planar, jp=jp)
        _nets[name, str(device)] = dict(nets=nets, J=J, meta=syn.make_meta(NET_B, NET_V, list(IMG)), maps=dict(
            planar=planar, nhwc=nhwc_heatmap_views(packed, J), nhwc_bf16=nhwc_heatmap_views(packed.bfloat16(), J)))
    return _nets[name, str(device)]


@contextlib.contextmanager
def _stub_v2v(rec):
    """V2VNet.forward writes down what it is handed and answers zeros of the right shape: the census ends at the opening conv"""
    from selfpose3d_amd.v2v_net import TiledZSpectrum, V2VNet
    inner = V2VNet.forward

    def forward(self, x):
        cout = self.output_layer.out_channels
        if isinstance(x, TiledZSpectrum):
            rec.calls.append(dict(fn="V2VNet", spectrum=_tensor(x.spec), SZ=x.SZ))
            return torch.zeros((x.shape[0], cout, x.X, x.Y, x.Z), device=x.device)
        rec.calls.append(dict(fn="V2VNet", input=_tensor(x)))
        y = torch.zeros((x.shape[0], cout) + tuple(x.shape[2:]), device=x.device)
        return y + 0 * x.reshape(-1)[0].float() if x.requires_grad else y
    V2VNet.forward = forward
    try:
        yield
    finally:
        V2VNet.forward = inner


def run_net_case(c, device):
    from selfpose3d_amd.project_layer import clear_pack_cache
    clear_pack_cache()
    s = _net_setup(c["cfg"], device)
    rec = Recorder()
    nets = s["nets"]
    for n in nets.values():          # every switch to its committed default, then the case's
        for name in SWITCH_NAMES:
            setattr(n.project_layer, name, False)
        n.project_layer.mode = "auto"
        n.v2v_net.one_front = n.v2v_net.wide_front = False
        n.v2v_net.fuse_zdft = True
    if c["kind"] == "pose":
        net = nets["pose"]
        net.project_layer.mode = c["mode"]
        gc = torch.zeros(NET_B, 4, 5, device=device)
        gc[:, :, :3] = torch.tensor(CENTER, device=device)
        gc[1, 1:, 3] = -1.0              # five valid proposals: one chunk of four and a tail of one
        hms = s["maps"]["nhwc"]
        rec.produced(hms)
        run = lambda: [_tensor(net.forward_batched(hms, s["meta"], gc, max_cubes_per_call=4))]
    elif c["kind"] == "train_rootnet":
        net = nets["soft"]
        rec.produced([])
        gen = torch.Generator().manual_seed(3)

        def run():
            with torch.enable_grad():
                return [_tensor(t) for t in net.train_rootnet(NET_B, s["meta"], generator=gen)]
    else:
        net = nets[c["net"]]
        front = NET_FRONTS[c["cfg"]]
        if front == "one":
            net.project_layer.one_zspectrum = net.v2v_net.one_front = c["front"]
        elif front == "wide":
            net.project_layer.wide_zspectrum = net.v2v_net.wide_front = c["front"]
        else:
            net.v2v_net.fuse_zdft = c["front"]
        net.project_layer.bf16_maps = c["bf16_maps"]
        net.project_layer.one_channel = bool(c.get("one_channel"))
        hms = s["maps"][c["hand"]]
        rec.produced(hms)

        def run():
            with (torch.enable_grad() if c["grad"] else torch.no_grad()):
                got = net(hms, s["meta"])
            return [None if t is None else _tensor(t) for t in got]

    def stubbed():
        with _stub_v2v(rec):
            return run()

    got = _outcome(rec, stubbed)
    clear_pack_cache()
    return got


def all_cases():
    """[(id, runner, case)] in the order the census file lists them"""
    return [(case_id(c), run_layer_case, c) for c in layer_cases()] + [(net_case_id(c), run_net_case, c) for c in net_cases()]
