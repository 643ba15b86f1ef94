"""CPU: the float64 model of the split-f16 evaluator (tests/f16x3_model.py) that tests/test_gpu_evaluator_range.py measures the
kernels against.  The packed operands unpack to the folded weights; every regime builder reaches the magnitudes it names;
the emulator (the format's own error) meets the bounds the GPU tests apply; and each deliberately wrong emulator (MUTANTS)
breaks them -- so those bounds would catch each of these faults in a kernel."""
import numpy as np
import pytest
import torch

import f16x3_model as M
from yinyang_game_alphazero_amd import network as N

R, C, CH, BLOCKS = 8, 8, 128, 10


@pytest.fixture(scope="module")
def planes():
    return M.encode(M.positions(R, C, 32, 1))


@pytest.fixture(scope="module")
def nets(planes):
    return {reg: M.make_net(reg, R, C, CH, BLOCKS, seed=1, planes=planes) for reg in M.REGIMES}


def _within_22_bits(hi, lo, want):
    """hi + lo == want to 22 significant bits, or to half the smallest float16 subnormal where lo is subnormal."""
    err = (hi + lo - want).abs()
    return bool((err <= torch.maximum(want.abs() * 2.0 ** -22, torch.full_like(want, 2.0 ** -25))).all())


@pytest.mark.parametrize("R_,C_,ch,blocks", [(8, 8, 128, 2), (5, 7, 96, 1), (1, 2, 64, 1), (9, 16, 32, 1), (11, 13, 128, 1)])
def test_packed_operands_unpack_to_the_folded_weights(R_, C_, ch, blocks):
    """pack_tower_g / pack_heads_g / pack_fc_heads read back through their documented layouts: each (hi, lo) equals
    split_f16 of the folded weight times 2^k, hi + lo equals w * 2^k to 22 bits, padded slots are zero."""
    net = M.make_net("calibrated", R_, C_, ch, blocks, seed=2)
    pk = M.Packed(net)
    for L, ((hi, lo), (conv, bn)) in enumerate(zip(pk.tower, N.tower_convs(net))):
        w, _ = N.fold_batchnorm(conv, bn)
        cin = w.shape[1]
        want = torch.ldexp(w.float(), torch.tensor(pk.kw))
        h16, l16 = N.split_f16(want)
        assert torch.equal(hi[:, :cin], h16.double()) and torch.equal(lo[:, :cin], l16.double()), L
        assert _within_22_bits(hi[:, :cin], lo[:, :cin], want.double()), L
        assert float(hi[:, cin:].abs().sum()) == 0.0 and float(lo[:, cin:].abs().sum()) == 0.0, L
    wp, _ = N.fold_batchnorm(net.policy_conv, net.policy_bn)
    wv, _ = N.fold_batchnorm(net.value_conv, net.value_bn)
    want = torch.ldexp(torch.cat([wp, wv]).float().reshape(64, -1), torch.tensor(pk.kh))
    assert _within_22_bits(pk.heads[0], pk.heads[1], want.double())
    assert torch.equal(pk.heads[0], N.split_f16(want)[0].double())
    for (hi, lo), lin in ((pk.fc_p, net.policy_fc), (pk.fc_v, net.value_fc1)):
        want = torch.ldexp(lin.weight.detach().float(), torch.tensor(pk.kf))
        assert torch.equal(hi, N.split_f16(want)[0].double()) and _within_22_bits(hi, lo, want.double())
    assert pk.fc_pad == 0.0
    assert pk.jobs[:, 2].max() <= 64 and int(pk.jobs[pk.jobs[:, 0] == 0, 2].sum()) == pk.A


def test_regime_builders_reach_their_magnitudes(nets, planes):
    """In float64 on the calibration positions: calibrated tops out near 10-30; small2 / small3 100x / 1000x below it; large
    in [2000, 8000]; wide holds gammas over 2^-14 .. 2^2 (some negative), dead channels (running_var 0), exactly zero output
    channels and all-zero input channels; saturated has logits spanning > 100 and |value pre-activation| > 10; flat equal
    logits; the overflow forms reach 8200 or more exactly where they name; the boundary net holds its channel at A."""
    ref = {k: M.reference_f64(n, planes) for k, n in nets.items()}
    top = {k: float(r["tower"].max()) for k, r in ref.items()}
    print({k: "%.3g" % v for k, v in top.items()})
    assert 5.0 < top["calibrated"] < 50.0
    assert top["calibrated"] / 300 < top["small2"] < top["calibrated"] / 30
    assert top["calibrated"] / 3000 < top["small3"] < top["calibrated"] / 300
    assert 2000.0 <= top["large"] <= 8000.0
    assert float(ref["large"]["feats"].max()) < 100.0
    w = nets["wide"]
    g = torch.cat([bn.weight.detach() for _, bn in N.tower_convs(w)])
    assert float(g.abs()[g != 0].min()) < 2.0 ** -13 and float(g.abs().max()) > 2.0 and bool((g < 0).any())
    for conv, bn in N.tower_convs(w):
        assert bool((bn.running_var == 0).any())
        assert bool((conv.weight.detach().flatten(1).abs().sum(1) == 0).any())
        assert bool((conv.weight.detach().transpose(0, 1).flatten(1).abs().sum(1) == 0).any())
        wf, bf = N.fold_batchnorm(conv, bn)
        assert bool(((wf.flatten(1).abs().sum(1) == 0) & (bf == 0)).any())      # an output channel that is exactly zero
    lg = ref["saturated"]["logits"]
    assert float((lg.max(1).values - lg.min(1).values).min()) > 100.0
    s = nets["saturated"]
    pre = torch.relu(ref["saturated"]["hidden"]) @ s.value_fc2.weight.detach().double().reshape(-1) + float(s.value_fc2.bias)
    assert float(pre.abs().min()) > 10.0
    lf = ref["flat"]["logits"]
    assert bool((lf == lf[:, :1]).all())
    for form in M.OVERFLOW_FORMS[1:]:
        r = M.reference_f64(M.make_net("overflow", R, C, 64, 4, seed=1, planes=planes, form=form), planes)
        where = {"network": r["tower"], "value_head": r["feats"][:, 1], "policy_head": r["feats"][:, 0]}[form]
        assert float(where.max()) >= 8200.0, form
        if form == "value_head":
            assert float(r["feats"][:, 0].max()) < 100.0
        if form == "policy_head":
            assert float(r["feats"][:, 1].max()) < 100.0
    assert float((M.poison_rows(planes, [3], "scale")[3]).max()) >= 8200.0
    for A in (8000.0, 8190.0):
        r = M.reference_f64(M.make_net("boundary", R, C, 64, 4, seed=1, planes=planes, boundary=A), planes)
        assert bool((r["tower"][:, 0] == A).all())


@pytest.mark.parametrize("regime", M.REGIMES)
def test_emulator_meets_the_gpu_bounds(regime, nets, planes):
    """The format's own error (emulator against float64) within F64_BOUNDS: whatever the kernels add is float32 accumulation
    order, bounded separately by EMU_BOUNDS on the GPU."""
    net = nets[regime]
    ref = M.reference_f64(net, planes)
    e = M.errors(M.emulate(M.Packed(net), planes), ref)
    e32 = M.errors(M.module_f32(net, planes), ref)
    print("%s emulator %s\n%s fp32 module %s" % (regime, e, regime, e32))
    bad = [(s, e[s], b) for s, b in M.F64_BOUNDS[regime].items() if not e[s] <= b]
    assert not bad, bad


# where each mutant must break the bounds (it may break them elsewhere too)
MUST_FAIL = {
    "drop_lo_hi": M.REGIMES,
    "bias_act_exp_plus_one": M.REGIMES,
    "flush_subnormals": ("small2", "small3", "wide"),          # tower per channel / tower_bias
    "truncate_split": ("small3",),
}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_each_mutant_breaks_the_bounds(mutant, nets, planes):
    """Deliberately wrong emulators: the lo*hi product dropped, float16 subnormals flushed to zero, truncation instead of
    round-to-nearest-even in the split, the bias scaled by 2^(ACT_EXP+1).  Each breaks F64_BOUNDS in the regimes listed in
    MUST_FAIL -- the GPU bounds would catch the same fault in a kernel."""
    broken = {}
    for regime in M.REGIMES:
        net = nets[regime]
        ref = M.reference_f64(net, planes)
        e = M.errors(M.emulate(M.Packed(net), planes, mutant), ref)
        bad = [s for s, b in M.F64_BOUNDS[regime].items() if not e[s] <= b]
        if bad:
            broken[regime] = {s: "%.2e > %.0e" % (e[s], M.F64_BOUNDS[regime][s]) for s in bad}
    print(mutant, broken)
    missed = [r for r in MUST_FAIL[mutant] if r not in broken]
    assert not missed, (mutant, missed)


def test_split_matches_the_product_split_and_the_mutants_differ():
    """split() is network.split_f16 bit for bit on normal, subnormal and boundary values; the mutant splits differ from it."""
    x = torch.tensor([0.0, 1.0, -1.0, 1.0 / 3.0, 1e-3, 3e-5, 6.1e-5, 1e-7, -2.5e-8, 1234.5678, 8189.9 * 8, np.pi * 1e-6],
                     dtype=torch.float32)
    hi, lo = M.split(x)
    h16, l16 = N.split_f16(x)
    assert torch.equal(hi, h16.double()) and torch.equal(lo, l16.double())
    assert not torch.equal(M.split(x, "flush_subnormals")[1], lo)
    assert not torch.equal(M.split(x, "truncate_split")[1], lo)
    inf_hi, inf_lo = M.split(torch.tensor([8190.0 * 8]))
    assert float(inf_hi) == float("inf") and float(inf_lo) == float("-inf")


def test_145_cells_are_not_covered():
    """A 145-cell board (5 x 29) is past the split-f16 kernels: f16x3_covers is False, mode "auto" picks "fp32" and "f16x3"
    refuses with ValueError (no device needed: both decisions are taken before anything is uploaded)."""
    net = M.make_net("calibrated", 5, 29, 32, 1, seed=3)
    assert not N.f16x3_covers(net)
    assert N.reference_precision_mode(net) == "fp32"
    with pytest.raises(ValueError):
        N.BatchedEvaluator(net, "f16x3")
