"""splat_slam_amd.update_op on the MI355X: the MFMA convolution bit for bit on exact data, and the whole operator against the fp64
statement tests/update_ref.py, its error measured against that of the torch autocast composition of the same weights.

Measured on an MI355X (max |error| of the kernels / of the torch composition, case (3,5,7) fp16): see DESIGN.md section 3, "Update
operator", and profiles/update_op_times.json."""
import os

import numpy as np
import pytest
import torch

import update_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 7
OUTS = ("net", "delta", "weight", "eta", "upmask")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_update_op.npz")


@pytest.fixture(scope="module")
def ops():
    from splat_slam_amd import update_op as U
    sd = U.synthetic_state_dict(SEED)
    return U.UpdateOperator.synthetic(SEED, DEV), R.TorchUpdate(sd, DEV), R.round_fp16(sd)


def eighths(g, shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 8.0


# ---- 1. exact convolution ---------------------------------------------------------------------------------------------------------
CONVS = [(196, 128, 1), (128, 128, 3), (4, 128, 7), (128, 64, 3), (448, 256, 3), (128, 2, 3), (128, 1, 3), (128, 576, 1)]
SIZES = [(1, 1, 1), (3, 5, 7), (5, 9, 13)]


@pytest.mark.parametrize("E,h,w", SIZES)
@pytest.mark.parametrize("cin,cout,k", CONVS)
def test_convolution_of_exact_data_equals_the_fp64_oracle_bit_for_bit(cin, cout, k, E, h, w):
    """inputs, weights and bias are multiples of 1/8 in [-1, 1], drawn independently (no two taps or channels alike): every product
    is a multiple of 1/64 and every partial sum stays below 2^24 / 64, so fp32 accumulation in any order is exact"""
    from splat_slam_amd.update_op import conv2d_f16
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + k)
    x, wt, b = eighths(g, (E, cin, h, w)), eighths(g, (cout, cin, k, k)), eighths(g, (cout,))
    got = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), out_dtype=torch.float32)
    ref = R.conv2d_ref(x, wt, b)
    assert got.dtype == torch.float32 and tuple(got.shape) == (E, cout, h, w)
    assert torch.equal(got.cpu().double(), ref)


@pytest.mark.parametrize("act", ["relu", "sigmoid", "tanh"])
def test_each_activation_of_an_exact_sum(act):
    """relu of an exact sum is exact; sigmoid and tanh are held to 4 fp32 ulp of the fp64 activation of the exact sum.  fp16 output
    is the correctly rounded fp32 result."""
    from splat_slam_amd.update_op import conv2d_f16
    g = torch.Generator().manual_seed(5)
    cin, cout, k = (128, 128, 3) if act == "relu" else (196, 128, 1)
    x, wt, b = eighths(g, (3, cin, 5, 7)), eighths(g, (cout, cin, k, k)), eighths(g, (cout,))
    got = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), act=act, out_dtype=torch.float32)
    ref = R.conv2d_ref(x, wt, b, act)
    if act == "relu":
        assert torch.equal(got.cpu().double(), ref) and (ref > 0).any() and (ref == 0).any()
    else:
        ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
        err = np.abs(got.cpu().double().numpy() - ref.numpy())
        print(act, "max error in ulp:", float((err / ulp).max()))
        assert (err <= 4 * ulp).all()
    half = conv2d_f16(x.to(DEV), wt.to(DEV), b.to(DEV), act=act)
    assert half.dtype == torch.float16 and torch.equal(half, got.half())


# ---- 2. halo isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,k", [(128, 128, 3), (4, 128, 7)])
def test_an_edge_reads_nothing_of_its_neighbours(cin, cout, k):
    from splat_slam_amd.update_op import conv2d_f16
    g = torch.Generator().manual_seed(k)
    x, wt = torch.randn(3, cin, 5, 7, generator=g).to(DEV), torch.randn(cout, cin, k, k, generator=g).to(DEV)
    a = conv2d_f16(x, wt)
    y = x.clone()
    y[1] = torch.randn(cin, 5, 7, generator=g).to(DEV)
    b = conv2d_f16(y, wt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


# ---- 3. the whole operator --------------------------------------------------------------------------------------------------------
def err(got, ref):
    d = (got.detach().double().cpu() - ref).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def check_against_oracle(name, hip, torch_out, oracle):
    """max |hip - oracle| <= 2 max |torch - oracle| and rms <= 1.5 rms, per output"""
    bad = []
    for n, a, b, o in zip(OUTS, hip, torch_out, oracle):
        (e_hip, r_hip), (e_ref, r_ref) = err(a, o), err(b, o)
        print(f"{name} {n}: max {e_hip:.3e} (torch {e_ref:.3e})  rms {r_hip:.3e} (torch {r_ref:.3e})")
        if not (e_hip <= 2 * e_ref and r_hip <= 1.5 * r_ref):
            bad.append((n, e_hip, e_ref, r_hip, r_ref))
    assert not bad, bad


def check_shapes(outs, E, K, h, w):
    assert tuple(outs[0].shape) == (1, E, 128, h, w) and outs[0].dtype == torch.float16
    assert tuple(outs[1].shape) == (1, E, h, w, 2) == tuple(outs[2].shape) and outs[1].dtype == outs[2].dtype == torch.float16
    if K:
        assert len(outs) == 5
        assert tuple(outs[3].shape) == (1, K, h, w) and outs[3].dtype == torch.float32
        assert tuple(outs[4].shape) == (1, K, 576, h, w) and outs[4].dtype == torch.float16
    else:
        assert len(outs) == 3
    for o in outs:
        assert o.is_contiguous() and torch.isfinite(o).all()


CASES = {"3x5x7-f16": (3, 5, 7, [2, 0, 2], torch.float16, False), "1x6x8-f32-no-ii": (1, 6, 8, None, torch.float32, False),
         "7x6x8-f16-strided": (7, 6, 8, [4, 1, 4, 1, 9, 4, 0], torch.float16, True), "7x6x8-f32": (7, 6, 8, [4, 1, 4, 1, 9, 4, 0], torch.float32, False)}


@pytest.mark.parametrize("case", list(CASES))
def test_operator_is_as_close_to_the_fp64_oracle_as_the_autocast_composition(ops, case):
    op, torch_op, sd16 = ops
    E, h, w, ii, dtype, strided = CASES[case]
    net, inp, corr, flow = R.make_inputs(E, h, w, seed=100 + E, device=DEV, dtype=dtype)
    if strided:
        big = torch.zeros(1, 2 * E, 128, h, w + 3, dtype=dtype, device=DEV)
        big[:, ::2, :, :, :w] = net
        net = big[:, ::2, :, :, :w]
        assert not net.is_contiguous()
    ii_t = None if ii is None else torch.tensor(ii, device=DEV)
    hip = op(net, inp, corr, flow, ii_t, None)
    check_shapes(hip, E, 0 if ii is None else len(set(ii)), h, w)
    ref = torch_op(net, inp, corr, flow, ii_t, None)
    oracle = R.update_ref(sd16, net, inp, corr, flow, None if ii is None else torch.tensor(ii))
    check_against_oracle(case, hip, ref, oracle)


def test_flow_none_is_zero_flow(ops):
    op = ops[0]
    net, inp, corr, flow = R.make_inputs(2, 5, 7, seed=3, device=DEV, dtype=torch.float16)
    a, b = op(net, inp, corr), op(net, inp, corr, torch.zeros_like(flow))
    assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 4. the fixture ---------------------------------------------------------------------------------------------------------------
def test_operator_on_the_reference_fixture(ops):
    """the recorded outputs of the reference's own module in float64 (unrounded weights), held to the bound of test 3"""
    op, torch_op, _ = ops
    g = np.load(GOLDEN)
    assert int(g["seed"]) == SEED
    ins = [torch.from_numpy(g["in_" + n]).to(DEV) for n in ("net", "inp", "corr", "flow")]
    ii = torch.from_numpy(g["ii"]).to(DEV)
    recorded = [torch.from_numpy(g["out_" + n]) for n in OUTS]
    check_against_oracle("fixture", op(*ins, ii, None), torch_op(*ins, ii, None), recorded)


# ---- 5. grouping ------------------------------------------------------------------------------------------------------------------
def test_permuting_the_edges_permutes_the_outputs(ops):
    """net, delta, weight are per edge: bitwise.  eta and upmask see the permutation only through the order of the fp32 sum of the
    segmented mean (group 4 has three edges): a reordering moves that sum by an fp32 rounding, which flips the fp16 rounding of the
    mean for about 1 element in 10^4, by 2^-11 |a| <= 2e-3 at |a| <= 4.  Through conv2 (|w| <= 1/sqrt(1152)) a flip moves 9 x 128
    hidden values by <= 6e-5 or one fp16 rounding of theirs (<= 5e-4 at |b| <= 1); through the 1x1 map (128 terms, |w| <= 0.088) that
    is <= 128 * 0.088 * 1e-4 ~ 1e-3 on upmask, held to 2e-3; through eta (0.01 softplus', 1152 terms, |w| <= 0.03) <= 5e-5."""
    op = ops[0]
    E, h, w, ii = 7, 6, 8, [4, 1, 4, 1, 9, 4, 0]
    net, inp, corr, flow = R.make_inputs(E, h, w, seed=21, device=DEV, dtype=torch.float16)
    perm = torch.tensor([3, 5, 0, 6, 2, 1, 4], device=DEV)
    ii_t = torch.tensor(ii, device=DEV)
    a = op(net, inp, corr, flow, ii_t)
    b = op(net[:, perm], inp[:, perm], corr[:, perm], flow[:, perm], ii_t[perm])
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x[:, perm], y)
    assert a[3].shape[1] == 4 == b[3].shape[1]
    d_eta, d_up = float((a[3] - b[3]).abs().max()), float((a[4].float() - b[4].float()).abs().max())
    print("eta", d_eta, "upmask", d_up)
    assert d_eta <= 5e-5 and d_up <= 2e-3


def test_groups_follow_sorted_unique_ii(ops):
    """with every group of size 1 a permutation leaves eta and upmask bitwise equal, and group k is the edge with the k-th smallest ii:
    its maps equal those of that edge run alone"""
    op = ops[0]
    E, h, w = 3, 5, 7
    net, inp, corr, flow = R.make_inputs(E, h, w, seed=22, device=DEV, dtype=torch.float16)
    ii = torch.tensor([7, 3, 5], device=DEV)
    a = op(net, inp, corr, flow, ii)
    perm = torch.tensor([2, 0, 1], device=DEV)
    b = op(net[:, perm], inp[:, perm], corr[:, perm], flow[:, perm], ii[perm])
    assert a[3].shape[1] == 3 and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for k, e in enumerate([1, 2, 0]):
        one = op(net[:, e:e + 1], inp[:, e:e + 1], corr[:, e:e + 1], flow[:, e:e + 1], ii[e:e + 1])
        assert torch.equal(one[3][0, 0], a[3][0, k]) and torch.equal(one[4][0, 0], a[4][0, k]) and torch.equal(one[0][0, 0], a[0][0, e])


# ---- 6. reproducibility and hygiene -----------------------------------------------------------------------------------------------
def test_calls_repeat_bit_for_bit_on_any_stream_and_leave_net_alone(ops):
    op = ops[0]
    E, h, w = 5, 9, 13
    net, inp, corr, flow = R.make_inputs(E, h, w, seed=31, device=DEV, dtype=torch.float16)
    ii = torch.tensor([1, 0, 1, 2, 0], device=DEV)
    keep = net.clone()
    a = op(net, inp, corr, flow, ii)
    b = op(net, inp, corr, flow, ii)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = op(net, inp, corr, flow, ii)
    side.synchronize()
    assert torch.equal(net, keep)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_bad_arguments_raise_before_any_launch(ops):
    op = ops[0]
    net, inp, corr, flow = R.make_inputs(2, 5, 7, seed=32, device=DEV, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        op(net.cpu(), inp, corr, flow)
    with pytest.raises(RuntimeError, match="196"):
        op(net, inp, corr[:, :, :195], flow)
    with pytest.raises(RuntimeError, match="empty"):
        op(net[:, :0], inp[:, :0], corr[:, :0], flow[:, :0])
    with pytest.raises(RuntimeError, match="ii"):
        op(net, inp, corr, flow, torch.tensor([0, 1, 2], device=DEV))


# ---- 7. in the graph --------------------------------------------------------------------------------------------------------------
N_FRAMES, HT, WD = 12, 48, 64


def make_video():
    """the recipe of tests/test_gpu_factor_graph.py: twelve keyframes on a smooth path in front of a gently varying surface"""
    from splat_slam_amd.depth_video import DepthVideo
    rng = np.random.default_rng(40)
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV).contiguous()
    v = DepthVideo(HT, WD, buffer=16, device=DEV)
    h, w = HT // 8, WD // 8
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for f in range(N_FRAMES):
        ang = 0.01 * f
        pose = np.array([0.03 * f, 0.01 * np.sin(f), 0.015 * f, 0.0, np.sin(ang / 2), 0.0, np.cos(ang / 2)])
        disp = 0.5 + 0.05 * np.sin(0.7 * xx + 0.3 * f) * np.cos(0.5 * yy) + rng.uniform(-0.005, 0.005, (h, w))
        v.append(float(f), torch.zeros(3, HT, WD, dtype=torch.uint8, device=DEV), f32(pose), f32(disp), None, f32([7.0, 7.5, 4.0, 3.0]))
    v.mono_disps[:N_FRAMES] = 1.7 * v.disps[:N_FRAMES] + 0.05
    v.fmaps[:N_FRAMES] = torch.tensor(rng.integers(-8, 9, size=(N_FRAMES, 1, 128, h, w)) / 8.0, dtype=torch.half, device=DEV)
    v.nets[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    v.inps[:N_FRAMES] = torch.tensor(rng.normal(size=(N_FRAMES, 128, h, w)), dtype=torch.half, device=DEV)
    return v


class Recorder:
    """an update operator that keeps the arguments and results of its first call"""

    def __init__(self, op):
        self.op, self.first = op, None

    def __call__(self, net, inp, corr, flow=None, ii=None, jj=None):
        out = self.op(net, inp, corr, flow, ii, jj)
        if self.first is None:
            self.first = ([t.clone() for t in (net, inp, corr, flow, ii)], [t.clone() for t in out])
        return out


@pytest.mark.parametrize("corr_impl", ["volume", "alt"])
def test_operator_drives_the_factor_graph(ops, corr_impl):
    from splat_slam_amd.factor_graph import FactorGraph
    op, torch_op, sd16 = ops
    runs = []
    for update_op in (Recorder(op), Recorder(torch_op)):
        v = make_video()
        g = FactorGraph(v, update_op, device=DEV, corr_impl=corr_impl, max_factors=-1)
        g.add_neighborhood_factors(0, 8 if corr_impl == "volume" else 12, r=2)
        E = g.ii.shape[0]
        if corr_impl == "volume":
            g.update(t0=1, itrs=2)
            if update_op.op is op:
                g.update(t0=1, itrs=2)
        else:
            g.update_lowmem(t0=1, t1=12, itrs=2, steps=2 if update_op.op is op else 1)
        if update_op.op is op:
            assert tuple(g.net.shape) == (1, E, 128, 6, 8) and g.net.dtype == torch.float16
            assert g.target.dtype == torch.float32 == g.weight.dtype and torch.isfinite(g.target).all() and torch.isfinite(g.weight).all()
            assert torch.isfinite(v.disps).all() and torch.isfinite(v.poses).all() and torch.isfinite(v.disps_up).all()
        runs.append(update_op.first)
    (ins_a, out_a), (ins_b, out_b) = runs
    assert all(torch.equal(x, y) for x, y in zip(ins_a, ins_b))                 # the first call sees the same inputs in both graphs
    net, inp, corr, flow, ii = ins_a
    oracle = R.update_ref(sd16, net.half(), inp.half(), corr.half(), flow.half(), ii.cpu())   # the oracle takes the fp16-rounded inputs
    check_against_oracle("graph-" + corr_impl, out_a, out_b, oracle)
