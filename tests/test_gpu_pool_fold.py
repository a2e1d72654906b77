"""The two residual convs that also write the MaxPool3d(2,2) of their result (SP3D_CONV3_POOL2X: _lib.conv3_split_ and
_lib.wino_fused_conv3d_ with pool=True), and the plan that uses them instead of its two maxpool2x launches.

Nothing here has a tolerance: with the flag the full result must be the bits of the same call without it (the same
accumulators, the same epilogue arithmetic), and the pooled tensor the bits of _lib.maxpool2x of that result (the same scan
order and comparison) - NaN positions compared with isnan, everything else as integers.  Outputs go into one NaN-filled buffer
with guard rows on both sides: an element the kernel never wrote stays NaN, a store outside its tensors breaks a guard.

Shapes (B, X, Y, Z).  Direct kernel (blocks of 16x8x4): one block; several blocks per sample and a batch boundary; 270 blocks,
more than the device has compute units, so a persistent workgroup walks a second block and the producer / consumer ring wraps.
Winograd kernel (blocks of 8x8x2, C = 64, CS = 32), both x forms: one block; blocks in all three axes and a batch boundary;
the half-resolution grid of the root net.

A sum of these kernels cannot be -0.0 (the accumulators start at +0.0, x + (-x) rounds to +0.0 and the ReLU writes +0.0), so the
-0.0 case feeds -0.0 inputs, zero weights for some outputs and a -0.0 shift and checks that whatever zeros come out pool to
the bits of the stand-alone kernel."""
import pytest
import torch

GUARD = 1024                                    # floats on either side of the outputs: 4 KB, keeps y 16-byte aligned
DIRECT = [(1, 16, 8, 4), (2, 32, 16, 8), (3, 80, 48, 12)]
WINO = [(1, 8, 8, 2), (2, 16, 24, 6), (1, 40, 40, 10)]
WIDTHS = {"direct": (32, 32, 16), "wino": (64, 64, 32)}            # (C, O, CS)
_cache = {}


def make_case(kind, shape):
    """inputs and weight records of a case, made once and never written"""
    key = (kind, shape)
    if key not in _cache:
        B, X, Y, Z = shape
        Cc, O, CS = WIDTHS[kind]
        g = torch.Generator().manual_seed(31 + X + 7 * Z)
        cl = torch.channels_last_3d
        c = dict(kind=kind, shape=shape,
                 h=torch.randn(B, Cc, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 xs=torch.randn(B, CS, X, Y, Z, generator=g).cuda().contiguous(memory_format=cl),
                 w2=(torch.randn(O, Cc, 3, 3, 3, generator=g) / (27 * Cc) ** 0.5).cuda(),
                 ws=(torch.randn(O, CS, 1, 1, 1, generator=g) / CS ** 0.5).cuda(),
                 shift=(0.5 * torch.randn(O, generator=g)).cuda())
        records(c)
        _cache[key] = c
    return _cache[key]


def records(c):
    from selfpose3d_amd import _lib
    Cc, O, CS = WIDTHS[c["kind"]]
    if c["kind"] == "direct":
        c["W"] = _lib.conv_weights_split(c["w2"])
        c["S"] = _lib.conv_weights_split(c["ws"])
    else:
        c["U"] = _lib.wino_weights(c["w2"])
        c["U3"] = _lib.wino_weights_split(c["U"], 16)
        c["U3yz"] = _lib.wino_yz_weights_split(c["w2"])
        c["S"] = _lib.wino_weights_split(c["ws"].reshape(O, CS).t().reshape(1, CS, O).contiguous(), 16)
    return c


def run(c, **kw):
    from selfpose3d_amd import _lib
    if c["kind"] == "direct":
        return _lib.conv3_split_(c["h"], c["W"], c["shift"], 1, xs=c["xs"], skip_w=c["S"], **kw)
    return _lib.wino_fused_conv3d_(c["h"], c["U"], c["shift"], 1, None, c["U3"], xs=c["xs"], skip_w=c["S"], U3yz=c["U3yz"], **kw)


def sizes(c):
    B, X, Y, Z = c["shape"]
    O = WIDTHS[c["kind"]][1]
    return B * X * Y * Z * O, B * (X // 2) * (Y // 2) * (Z // 2) * O


def flat(t):
    """the memory of a channels_last_3d tensor, in order"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1)


def same_bits(a, b):
    """NaN in the same places, the same bits everywhere else"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb]))


def guarded(c):
    n, npool = sizes(c)
    buf = torch.full((GUARD + n + npool + GUARD,), float("nan"), device="cuda")
    return buf, buf[GUARD:GUARD + n + npool]


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def check_case(c, expect_nan=False):
    from selfpose3d_amd import _lib
    n, npool = sizes(c)
    plain = run(c)
    want_pool = _lib.maxpool2x(plain)
    buf, out = guarded(c)
    y, yp = run(c, pool=True, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr() and yp.data_ptr() == out.data_ptr() + 4 * n
    assert y.shape == plain.shape and y.stride() == plain.stride() and yp.shape == want_pool.shape and yp.stride() == want_pool.stride()
    assert guards_intact(buf), "a store outside the two tensors"
    if not expect_nan:
        assert not bool(torch.isnan(out).any()), "an element the kernel never wrote"
        assert torch.equal(out[:n].view(torch.int32), flat(plain).view(torch.int32))
        assert torch.equal(out[n:].view(torch.int32), flat(want_pool).view(torch.int32))
    assert same_bits(out[:n], flat(plain)), "y differs from the call without the flag"
    assert same_bits(out[n:], flat(want_pool)), "y_pooled differs from maxpool2x(y)"
    # and the pooled tensor is torch's pooling of that result (NaN propagates in both)
    ref = torch.nn.functional.max_pool3d(plain, 2, 2)
    assert same_bits(out[n:], flat(ref.contiguous(memory_format=torch.channels_last_3d)))
    return plain, yp


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    monkeypatch.delenv("SP3D_FOLD_SKIP", raising=False)
    monkeypatch.delenv("SP3D_WINO_YZ", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DIRECT, ids=lambda s: "x".join(map(str, s)))
def test_direct_pooled_is_plain_plus_maxpool(shape):
    plain, yp = check_case(make_case("direct", shape))
    pos = float((plain > 0).float().mean())
    assert 0.1 <= pos <= 0.9, pos                    # the ReLU cuts some and passes some: the cells mix zeros and values


@pytest.mark.gpu
@pytest.mark.parametrize("yz", [False, True], ids=["x_winograd", "x_direct"])
@pytest.mark.parametrize("shape", WINO, ids=lambda s: "x".join(map(str, s)))
def test_wino_pooled_is_plain_plus_maxpool(shape, yz, monkeypatch):
    monkeypatch.setenv("SP3D_WINO_YZ", "1" if yz else "0")
    plain, yp = check_case(make_case("wino", shape))
    pos = float((plain > 0).float().mean())
    assert 0.1 <= pos <= 0.9, pos


def _variant(kind, shape, edit):
    c = dict(make_case(kind, shape))
    for k in ("h", "xs", "w2", "ws", "shift"):
        c[k] = c[k].clone()
    edit(c)
    return records(c)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape,yz", [("direct", DIRECT[1], False), ("wino", WINO[1], False), ("wino", WINO[1], True)],
                         ids=["direct", "wino_x_winograd", "wino_x_direct"])
def test_nan_in_a_cell_propagates_like_the_pool_kernel(kind, shape, yz, monkeypatch):
    monkeypatch.setenv("SP3D_WINO_YZ", "1" if yz else "0")

    def edit(c):
        # a NaN in the projection's input: every channel of that voxel is NaN (the folded ReLU keeps it), at each position
        # of a cell in turn - first, middle and last of the scan - and across a block and a batch boundary
        B, X, Y, Z = shape
        for b, x, y, z in ((0, 0, 0, 0), (0, 3, 2, 1), (0, X - 1, Y - 1, Z - 1), (B - 1, 8, 7, 2), (B - 1, 9, 8, 3)):
            c["xs"][b, 5, x, y, z] = float("nan")
    c = _variant(kind, shape, edit)
    plain, yp = check_case(c, expect_nan=True)
    assert int(torch.isnan(plain).sum()) == 5 * WIDTHS[kind][1]
    nanp = torch.isnan(yp)
    assert int(nanp.sum()) == 5 * WIDTHS[kind][1]                # five different cells, every channel
    assert bool(nanp[0, :, 0, 0, 0].all()) and bool(nanp[shape[0] - 1, :, 4, 3, 1].all()) and bool(nanp[shape[0] - 1, :, 4, 4, 1].all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("direct", DIRECT[1]), ("wino", WINO[1])], ids=["direct", "wino"])
def test_zeros_of_either_sign_pool_like_the_pool_kernel(kind, shape):
    def edit(c):
        O = WIDTHS[kind][1]
        c["w2"][: O // 2] = 0.0                      # half the outputs: shift alone, -0.0 / +0.0 / a negative value
        c["ws"][: O // 2] = 0.0
        c["shift"][: O // 2] = torch.tensor([-0.0, 0.0, -1.0, -0.0] * (O // 8), device="cuda")
        c["h"][:, :, ::2] = -0.0                     # ... and signed zeros among the inputs of the others
        c["xs"][:, :, :, ::3] = -0.0
    c = _variant(kind, shape, edit)
    plain, yp = check_case(c)
    assert bool((plain[:, : WIDTHS[kind][1] // 2] == 0).all())      # whole cells of zeros: ties at every step of the scan


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", [("direct", (2, 20, 12, 6)), ("direct", (1, 16, 8, 6)), ("wino", (2, 12, 10, 3)),
                                        ("wino", (1, 8, 12, 2))], ids=["direct_all_axes", "direct_z", "wino_all_axes", "wino_y"])
def test_ragged_grid_is_refused_and_nothing_is_written(kind, shape):
    from selfpose3d_amd import _lib
    c = make_case(kind, shape)
    assert not _lib.pool_fold_covers("conv3_split_" if kind == "direct" else "wino_fused_conv3d_", *shape[1:])
    buf, out = guarded(c)
    with pytest.raises(_lib.Sp3dError, match="not supported|unsupported|code -4"):
        run(c, pool=True, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    run(c)                                           # the plain call takes the grid as before
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_pool_without_the_folded_skip_is_an_error():
    from selfpose3d_amd import _lib
    c = make_case("direct", DIRECT[0])
    with pytest.raises(_lib.Sp3dError):
        _lib.conv3_split_(c["h"], c["W"], c["shift"], 1, pool=True)
    w = make_case("wino", WINO[0])
    with pytest.raises(_lib.Sp3dError):
        _lib.wino_fused_conv3d_(w["h"], w["U"], w["shift"], 1, None, w["U3"], pool=True)
    with pytest.raises(_lib.Sp3dError):
        run(c, pool=True, out=torch.empty(sum(sizes(c)) + 1, device="cuda"))


# ---- the plan -----------------------------------------------------------------------------------------------------------
def make_net(cout, seed):
    """a V2VNet with unit-gain weights (in the fresh net, std 0.001, a conv term fades below an ulp of its shift), on the GPU
    in the layout the plan's kernels run in"""
    from selfpose3d_amd.v2v_net import V2VNet
    torch.manual_seed(seed)
    net = V2VNet(15, cout)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._NormBase):
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.num_features, generator=g))
            elif isinstance(m, torch.nn.ConvTranspose3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[0] ** 0.5)
            elif isinstance(m, torch.nn.Conv3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight[0].numel() ** 0.5)
    net.eval().cuda().to(memory_format=torch.channels_last_3d)
    return net, g


class PoolLaunches:
    """counts the launches of maxpool2x_cl_kernel at the ctypes entry (no profiler)"""

    def __init__(self, monkeypatch):
        from selfpose3d_amd import _lib
        lib = _lib.load()
        inner = lib.sp3d_maxpool2x_cl
        self.n = 0

        def counted(*a):
            self.n += 1
            return inner(*a)
        monkeypatch.setattr(lib, "sp3d_maxpool2x_cl", counted)


PLANS = {"root_80x80x20": (1, (1, 15, 80, 80, 20), 41), "pose_64": (15, (1, 15, 64, 64, 64), 43)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANS))
def test_plan_with_folded_pools_is_the_plan_without_bit_for_bit(name, monkeypatch):
    cout, shape, seed = PLANS[name]
    net, g = make_net(cout, seed)
    x = torch.rand(shape, generator=g).cuda()
    count = PoolLaunches(monkeypatch)
    monkeypatch.setenv("SP3D_FOLD_POOL", "0")
    with torch.no_grad():
        y_off = net(x).clone()
    torch.cuda.synchronize()
    assert count.n == 2
    monkeypatch.setenv("SP3D_FOLD_POOL", "1")
    with torch.no_grad():
        y_on = net(x).clone()
    torch.cuda.synchronize()
    assert count.n == 2, "a maxpool2x_cl launch with the pools folded"
    assert net._get_plan().pooled is None                    # handed over and dropped
    assert y_on.shape == y_off.shape and y_on.stride() == y_off.stride()
    assert bool(torch.isfinite(y_off).all()) and float(y_off.abs().max()) > 1e-3
    assert torch.equal(y_on.view(torch.int32), y_off.view(torch.int32))


@pytest.mark.gpu
def test_graph_replay_of_the_folded_plan_is_eager(monkeypatch):
    monkeypatch.setenv("SP3D_FOLD_POOL", "1")
    net, g = make_net(1, 47)
    x = torch.rand((1, 15, 80, 80, 20), generator=g).cuda()
    count = PoolLaunches(monkeypatch)
    with torch.no_grad():
        eager = net(x).clone()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(x)                                            # the side stream's first touch of every buffer, uncaptured
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(x)
        out.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert count.n == 0
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
