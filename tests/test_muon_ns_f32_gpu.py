"""Muon(ns_dtype="float32"): the Newton-Schulz chain in exact fp32 (csrc/muon_ns_f32.hip) against the
reference's arithmetic.

The bound comes from the reference, not from the code under test: for every routed leaf and step,
``d_ref`` is the rel-Frobenius distance of the fp32 CPU oracle's update from the fp64 oracle's on the
same gradients, and the device's distance from the fp64 oracle must be <= 4 x d_ref (the device sums
every dot product in another order and blocking than the CPU; permuting the contraction order on the
CPU moves d_ref by under 10 %).  d_ref is 1e-6 .. 2e-6 for shapes up to 256 on a side and ~3e-5 at
768 x 2048, three to four orders of magnitude below the bf16 chain's 1e-2, which the teeth test
requires to miss the same bound by more than 100 x.  Each test prints its per-leaf ratios
d_dev / d_ref.  Through ``step_`` the update is seen as p_after - p_before, which carries the fp32
rounding of p + u (half an ulp of p, ~5e-6 of the update here): step_rel subtracts that floor, so the
``step_`` cases resolve the chain's error only above it (they still catch the bf16 chain, a wrong
gscale, a missed apply or shadow) and the ``update`` cases carry the tight comparison.

Measured on an MI355X: worst d_dev / d_ref 1.07 over every fp32 case (dense shapes 0.49 .. 1.06,
lm768 0.13, ns_steps = 0 1.07, schedule-free 0.99); the bf16 chain 6.5e3 .. 3.0e4.
"""
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.parity_util import ADAM_TOL, rel, routed, step_rel
from tests.test_optim_parity_gpu import LAYOUTS, _grads, run_pair

FACTOR = 4.0
LR, WD = 1e-2, 0.1
KW = dict(weight_decay=WD, adam_b1=0.9, adam_b2=0.95, adam_weight_decay=WD)

# (7, 33) / (33, 7): one partial tile, K not a multiple of 4, transposed; the ViT's own shapes;
# (130, 258): just past every 128 / 256 boundary (and past the K = 128 boundary of the per-wave K
# split: 16 -> 32 columns per wave); (32, 64) / (33, 65): either side of the 32-wide tile edge
SHAPES = [(7, 33), (33, 7), (48, 100), (200, 64), (96, 256), (128, 256), (256, 128), (128, 200), (130, 258),
          (32, 64), (33, 65)]


def _dense_layout():
    from plaincv_amd.params import Layout
    lay = Layout()
    for i, s in enumerate(SHAPES):
        lay.add(f"Dense_{i}/kernel", s)
    lay.add("Dense_0/bias", (33,))     # the Adam branch runs too
    return lay


class DualOracle:
    """The fp64 and the fp32 CPU oracle on the same gradients, each on its own trajectory.  run_pair
    sees the fp64 updates; the fp32 ones are kept in ``u32`` (one dict per step)."""

    def __init__(self, make):
        self.tx64, self.tx32, self.u32 = make(), make(), []

    def init(self, params):
        self.p64 = OrderedDict((k, v.double()) for k, v in params.items())
        self.p32 = OrderedDict((k, v.clone()) for k, v in params.items())
        self.s64, self.s32 = self.tx64.init(self.p64), self.tx32.init(self.p32)
        return None

    def update(self, grads, state, params):
        u64, self.s64 = self.tx64.update(OrderedDict((k, g.double()) for k, g in grads.items()), self.s64, self.p64)
        u32, self.s32 = self.tx32.update(grads, self.s32, self.p32)
        for k in u64:
            assert u64[k].dtype == torch.float64 and u32[k].dtype == torch.float32, k
            self.p64[k] = self.p64[k] + u64[k]
            self.p32[k] = self.p32[k] + u32[k]
        self.u32.append(u32)
        return u64, None


def ratios(steps, u32s, tag):
    """Per routed leaf the worst d_dev / d_ref over the steps (printed); the worst Adam-branch error."""
    out, wa = OrderedDict(), 0.0
    for (hip, u64, p0, p1), u32 in zip(steps, u32s):
        for k in u64:
            d_dev = rel(hip[k], u64[k]) if p0 is None else step_rel(p0[k], p1[k], u64[k])
            if routed(k, u64[k]):
                d_ref = rel(u32[k], u64[k])
                assert d_ref > 0.0, k
                out[k] = max(out.get(k, 0.0), d_dev / d_ref)
            else:
                wa = max(wa, d_dev)
    for k, r in out.items():
        print(f"NS_F32 {tag} {k} d_dev/d_ref {r:.3f}")
    print(f"NS_F32 {tag} worst {max(out.values()):.3f} adam {wa:.3e}")
    return out, wa


def _pair(dev, layout, gpu_tx, make_oracle, steps, mode, gscale, tag):
    ora = DualOracle(make_oracle)
    res = run_pair(dev, layout, gpu_tx, ora, steps, mode, gscale)
    return ratios(res, ora.u32, tag)


def _muon(**kw):
    from plaincv_amd.optim.muon import Muon
    return Muon(LR, **{**KW, **kw})


def _oracle(**kw):
    from oracle import optim as oopt
    return lambda: oopt.muon(LR, **{**KW, **kw})


MODES = [("update", 1.0), ("step_", 0.37)]


@pytest.mark.parametrize("mode,gscale", MODES)
def test_accuracy_against_reference_arithmetic(dev, mode, gscale):
    r, wa = _pair(dev, _dense_layout(), _muon(ns_dtype="float32"), _oracle(), 3, mode, gscale, f"dense {mode}")
    assert len(r) == len(SHAPES)
    assert max(r.values()) <= FACTOR, r
    assert wa <= ADAM_TOL, wa


@pytest.mark.parametrize("mode,gscale", MODES)
def test_bf16_chain_misses_the_bound_by_far(dev, mode, gscale):
    """Teeth: the default bf16 chain under the same rule."""
    r, _ = _pair(dev, _dense_layout(), _muon(ns_dtype="bfloat16"), _oracle(), 3, mode, gscale, f"bf16 {mode}")
    assert min(r.values()) > 100 * FACTOR, r


@pytest.mark.parametrize("mode,gscale", MODES)
def test_lm_shapes(dev, mode, gscale):
    """768 x 2304, the fused 768 x 2048 pair, 2048 x 768: many tiles per matrix, long K."""
    r, wa = _pair(dev, LAYOUTS["lm768"](), _muon(ns_dtype="float32"), _oracle(), 2, mode, gscale, f"lm768 {mode}")
    assert max(r.values()) <= FACTOR, r
    assert wa <= ADAM_TOL, wa


@pytest.mark.parametrize("mode,gscale", MODES)
@pytest.mark.parametrize("variant", ["adaptive", "no_nesterov", "ns_steps_0", "no_shape_scale"])
def test_variants_on_the_vit_layout(dev, variant, mode, gscale):
    kw = {"adaptive": dict(adaptive=True), "no_nesterov": dict(nesterov=False), "ns_steps_0": dict(ns_steps=0),
          "no_shape_scale": dict(shape_scale=False)}[variant]
    okw = dict(kw)
    if variant == "no_nesterov":      # optax.contrib.muon's flag also switches the Adam branch
        okw["adam_nesterov"] = False
    r, wa = _pair(dev, LAYOUTS["vit_c2"](), _muon(ns_dtype="float32", **kw), _oracle(**okw), 3, mode, gscale,
                  f"{variant} {mode}")
    assert max(r.values()) <= FACTOR, r
    assert wa <= ADAM_TOL, wa
    if variant == "adaptive":         # against the non-adaptive oracle it must fail by far
        r, _ = _pair(dev, LAYOUTS["vit_c2"](), _muon(ns_dtype="float32", **kw), _oracle(), 2, mode, gscale,
                     f"adaptive-vs-plain {mode}")
        assert min(r.values()) > 100 * FACTOR, r


def test_schedule_free_wrapper(dev):
    from oracle import optim as oopt
    from plaincv_amd.optim.schedule_free import ScheduleFree
    gpu = ScheduleFree(_muon(ns_dtype="float32"), 0.03, 0.9, 2.0)
    r, wa = _pair(dev, LAYOUTS["vit_c2"](), gpu, lambda: oopt.schedule_free(_oracle()(), 0.03, 0.9, 2.0), 3, "update",
                  1.0, "schedule_free")
    assert max(r.values()) <= FACTOR, r
    assert wa <= ADAM_TOL, wa


def _fresh(dev, layout, seed=0):
    from plaincv_amd.params import ParamStore
    gen = torch.Generator().manual_seed(seed)
    store = ParamStore(layout, dev)
    store.load(OrderedDict((k, 0.1 * torch.randn(l.shape, generator=gen)) for k, l in layout.leaves.items()))
    return store


def _set_grads(store, grads, dev):
    store.zero_grad()
    for k, v in grads.items():
        store.grads[k].copy_(v.to(dev))


def _state_equal(sa, sta, sb, stb):
    assert torch.equal(sa.flat, sb.flat)
    assert torch.equal(sa.shadow, sb.shadow)
    for name in ("mu", "nu"):
        assert torch.equal(sta.tensors[name], stb.tensors[name]), name
    assert torch.equal(sta.count, stb.count)


def test_two_runs_give_identical_bits(dev):
    lay = LAYOUTS["vit_c2"]()
    gen = torch.Generator().manual_seed(1)
    grads = [_grads(lay, gen, {k: 0.1 for k in lay.leaves}) for _ in range(3)]
    runs = []
    for _ in range(2):
        tx = _muon(ns_dtype="float32")
        store = _fresh(dev, lay)
        st = tx.init(store)
        for g in grads:
            _set_grads(store, g, dev)
            tx.step_(store, st)
        torch.cuda.synchronize()
        runs.append((store, st))
    _state_equal(*runs[0], *runs[1])
    assert int(runs[0][1].count.item()) == 3


@pytest.mark.parametrize("rank", [0, 1])
def test_sharded_rank_runs_its_own_matrices(dev, rank, monkeypatch):
    """shard=(rank, 2): the rank's records, workspaces and tile table cover only the matrices it owns.
    With the post-step broadcast stubbed out (one process, no process group), the owned matrices and the
    replicated Adam-branch leaves get the unsharded step's bits and the other routed matrices stay put."""
    from plaincv_amd.optim import sharding
    monkeypatch.setattr(sharding, "finish", lambda *a, **k: None)
    lay = LAYOUTS["vit_c2"]()
    gen = torch.Generator().manual_seed(3)
    g = _grads(lay, gen, {k: 0.1 for k in lay.leaves})
    full, part = _muon(ns_dtype="float32"), _muon(ns_dtype="float32", shard=(rank, 2))
    sa, sb = _fresh(dev, lay), _fresh(dev, lay)
    sta, stb = full.init(sa), part.init(sb)
    owned = set(stb.routed)
    assert 0 < len(owned) < len(sta.routed) and not part.split_capable(stb)
    before = sb.to_dict()
    for tx, store, st in ((full, sa, sta), (part, sb, stb)):
        _set_grads(store, g, dev)
        tx.step_(store, st)
    torch.cuda.synchronize()
    pa, pb = sa.to_dict(), sb.to_dict()
    for k in pa:
        if k in sta.routed and k not in owned:
            assert torch.equal(pb[k], before[k]), k
        else:
            assert torch.equal(pb[k], pa[k]), k


def test_step_replays_from_a_captured_graph(dev):
    """step_ is a fixed launch sequence (no host reads, no allocation after init): captured once and
    replayed three times it gives the bits of three eager steps."""
    lay = LAYOUTS["vit_c2"]()
    gen = torch.Generator().manual_seed(2)
    g = _grads(lay, gen, {k: 0.1 for k in lay.leaves})
    gs = torch.full((1,), 0.37, device=dev)
    tx = _muon(ns_dtype="float32")
    sa, sb = _fresh(dev, lay), _fresh(dev, lay)
    sta, stb = tx.init(sa), tx.init(sb)
    _set_grads(sa, g, dev)
    _set_grads(sb, g, dev)
    for _ in range(3):                 # eager (also loads every kernel before the capture)
        tx.step_(sa, sta, gscale=gs)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        tx.step_(sb, stb, gscale=gs)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    _state_equal(sa, sta, sb, stb)
    assert int(stb.count.item()) == 3


@pytest.mark.parametrize("aligned", [False, True])
def test_graphed_step_optimizer_overlap_f32(dev, aligned):
    """tests/test_vit_parity_gpu.py test_graphed_step_optimizer_overlap with muon_ns_dtype="float32":
    GraphedTrainStep(overlap_opt=True) (split step: gradient phase, then the fp32 chain + apply + bump
    on the side stream) against the in-step optimizer, bitwise."""
    from plaincv_amd.engine import GraphedTrainStep, create_train_state
    from plaincv_amd.models.vit_small import VisionTransformer
    from utils import Config
    m = VisionTransformer(num_classes=16 if aligned else 10, patch_size=4, hidden_size=64, mlp_dim=128,
                          num_layers=2, num_heads=2, dropout_rate=0.1)
    shape = (8, 16, 16, 3)
    cfg = Config(optim="muon", lr=1e-3, weight_decay=0.01, beta1=0.9, beta2=0.9, muon_ns_dtype="float32")
    init = m.init(5, shape)
    g = torch.Generator().manual_seed(7)
    xs = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8).to(dev)
    ys = torch.randint(0, 10, (3, shape[0]), generator=g, dtype=torch.int32).to(dev)
    sa = create_train_state(0, m, 1e-3, shape, 10, cfg=cfg, init_params=init)
    sb = create_train_state(0, m, 1e-3, shape, 10, cfg=cfg, init_params=init)
    assert sa.tx.ns_dtype == "float32" and sb.tx.ns_dtype == "float32"
    ga = GraphedTrainStep(sa, shape, warmup=2, overlap_opt=True)
    gb = GraphedTrainStep(sb, shape, warmup=2)
    assert ga.overlap and not gb.overlap
    assert sa.opt_state.vec4 == aligned
    gb.runner.seed.copy_(ga.runner.seed)
    for it in range(6):
        k = it % 3
        ma = ga(xs[k], ys[k]).clone()
        mb = gb(xs[k], ys[k]).clone()
        torch.cuda.synchronize()
        assert torch.equal(ma, mb), (it, ma, mb)
        if it == 3:   # a flush mid-run, then the first (non-steady) graph again
            ga.flush()
            torch.cuda.synchronize()
            assert torch.equal(sa.params.flat, sb.params.flat), it
    assert sa.params.pending is not None
    pa = sa.params.to_dict()
    assert sa.params.pending is None and not ga.pending
    pb = sb.params.to_dict()
    diff = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not diff, diff
    assert torch.equal(sa.params.shadow, sb.params.shadow)
    for name in ("mu", "nu"):
        assert torch.equal(sa.opt_state.tensors[name], sb.opt_state.tensors[name]), name
    assert torch.equal(sa.opt_state.count, sb.opt_state.count)
    assert int(sa.opt_state.count.item()) > 0
