"""GPU: the split-f16 evaluator ("f16x3": csrc/yy_tower_g.hip, yy_fc_heads.hip, k_head_finish_f32) at the edges of its number
format and of its kernel geometry, against the float64 module and against the float64 emulator of its own arithmetic
(tests/f16x3_model.py).  Errors are measured per output channel (f16x3_model.channel_error), stage by stage: tower
activations, head features, logits / value_fc1 output, policy / value.  Bounds: f16x3_model.F64_BOUNDS (kernel against
float64) and EMU_BOUNDS (kernel against the emulator: float32 accumulation order only); the measured values are printed
and listed in each test's docstring.  Overflow: an activation of 8190 or more (times 2^ACT_EXP = 65520, float16 infinity)
must come out as NaN in exactly the rows it touches, and a search fed such a network must raise YYError."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACC_SHAPES = [(8, 8, 128), (12, 12, 128), (6, 6, 128)]
GEO_SHAPES = [(1, 1, 32), (1, 2, 64), (2, 8, 32), (7, 9, 96), (5, 13, 64), (11, 13, 128), (9, 16, 32), (16, 9, 128)]


def _pkg():
    import yinyang_game_alphazero_amd as pkg
    return pkg


def _kernel_stages(ev, planes):
    """Every stage of the f16x3 evaluator on planes (cuda): the tower alone, the tower + fused head convolutions, the FC
    heads kernel on those features and the evaluator's own (policy, value)."""
    E = _pkg().engine
    nb, tb = ev.g_big
    tower = E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb)
    feats = E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb, ev.g_hw, ev.g_hb)
    logits, hidden = E.fc_heads(feats, ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps)
    p, v = ev(planes)
    return dict(tower=tower, feats=feats, logits=logits, hidden=hidden, policy=p, value=v)


def _fmt(e):
    return " ".join("%s %.2e" % kv for kv in e.items())


def _check_accuracy(M, net, planes, regime, label, mode="f16x3"):
    import torch
    pkg = _pkg()
    ev = pkg.BatchedEvaluator(net.cuda().eval(), mode)
    if mode == "f16x3r":
        E = pkg.engine
        got = dict(tower=E.tower_forward_h3r(planes, ev.h3r_w, ev.h3_b[:ev.h3_layers].contiguous(), ev.h3_layers, ev.h3_exps),
                   feats=E.tower_heads_forward_h3r(planes, ev.h3r_w, ev.h3r_hw, ev.h3_b, ev.h3_layers, ev.h3_exps))
        got["logits"], got["hidden"] = E.fc_heads(got["feats"], ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps)
        got["policy"], got["value"] = ev(planes)
    else:
        assert ev.mode == "f16x3"
        got = _kernel_stages(ev, planes)
    for t in got.values():
        assert bool(torch.isfinite(t).all())
    ref = M.reference_f64(net, planes)
    emu = M.emulate(M.Packed(net), planes)
    f32 = M.module_f32(net, planes)
    e64, eemu, e32, fmt64 = M.errors(got, ref), M.errors(got, emu), M.errors(f32, ref), M.errors(emu, ref)
    print("\n%s %s [max tower %.3g]\n  kernel-f64 %s\n  kernel-emu %s\n  emu-f64    %s\n  fp32-f64   %s" % (
        label, mode, float(ref["tower"].max()), _fmt(e64), _fmt(eemu), _fmt(fmt64), _fmt(e32)))
    bad = [(s, e64[s], b) for s, b in M.F64_BOUNDS[regime].items() if not e64[s] <= b]
    bad += [("emu " + s, eemu[s], b) for s, b in M.EMU_BOUNDS[regime].items() if not eemu[s] <= b]
    assert not bad, bad


@pytest.mark.parametrize("regime", ["calibrated", "small2", "small3", "large", "wide", "saturated", "flat"])
@pytest.mark.parametrize("R,C,ch", ACC_SHAPES)
def test_f16x3_accuracy_per_regime(regime, R, C, ch):
    """Each regime of f16x3_model (BN statistics from real positions; tower gamma / beta times 1e-2 and 1e-3; a tower top in
    [3000, 7000]; gammas over 2^-14 .. 2^2 with negative, dead and zero channels; saturated and flat heads) on the 128 x 10
    network: the kernels against float64 within F64_BOUNDS and against the emulator within EMU_BOUNDS, every stage, per
    output channel.  Measured (8x8 / 12x12 / 6x6): policy within 1.6e-6 of float64 in every regime (bound 2e-6; the fp32
    module 2.1e-6); value within 4.4e-6 (bound 1e-5; the fp32 module 6.6e-6 on the same inputs: value_fc1 sums 2 048 -
    4 608 products, float32 accumulation alone exceeds 2e-6 there); per channel, tower / features / logits / hidden within
    2.8e-6 / 3.0e-6 / 4.3e-6 / 5.5e-6 except in the small regimes, where the format's own error dominates (small3 tower
    2.5e-3 per channel, equal to the emulator's: activations near 2^-20 keep only subnormal lo bits).  Kernel against the
    emulator: 2.8e-6 per channel and 4.8e-6 on value outside the small regimes."""
    import torch
    import f16x3_model as M
    planes = M.encode(M.positions(R, C, 64, 11))
    net = M.make_net(regime, R, C, ch, 10, seed=2, planes=planes, device="cuda")
    _check_accuracy(M, net, planes.cuda(), regime, "%s %dx%d c%d" % (regime, R, C, ch))
    torch.cuda.synchronize()


@pytest.mark.parametrize("R,C,ch,blocks", [(5, 7, 96, 4), (9, 12, 32, 4)])
def test_f16x3_accuracy_calibrated_other_widths(R, C, ch, blocks):
    """The calibrated regime on non-square boards at 96 and 32 channels: bounds as test_f16x3_accuracy_per_regime."""
    import f16x3_model as M
    planes = M.encode(M.positions(R, C, 64, 12))
    net = M.make_net("calibrated", R, C, ch, blocks, seed=4, planes=planes)
    _check_accuracy(M, net, planes.cuda(), "calibrated", "calibrated %dx%d c%d" % (R, C, ch))


def test_f16x3r_accuracy_calibrated():
    """Mode "f16x3r" (csrc/yy_tower_h3r.hip, the 32x32x16 tower) on the calibrated 8x8 128 x 10 network: the same packed
    values and arithmetic as the general kernel, so the same bounds."""
    import f16x3_model as M
    planes = M.encode(M.positions(8, 8, 64, 13))
    net = M.make_net("calibrated", 8, 8, 128, 10, seed=5, planes=planes)
    _check_accuracy(M, net, planes.cuda(), "calibrated", "calibrated 8x8 c128", mode="f16x3r")


def _forms(R, C, ch):
    E = _pkg().engine
    out = []
    for nb in E.tower_g_available(ch):
        tb_max = (16 * nb) // (R * C)
        for tb in sorted({1, tb_max}) if tb_max else ():
            out.append((nb, tb))
    return out


@pytest.mark.parametrize("R,C,ch", GEO_SHAPES)
def test_f16x3_geometry_edges_match_the_emulator(R, C, ch):
    """Boards of 1, 2, 16 (2x8: one 4-block form exactly full), 63, 65, 143 and 144 cells (square and not), every width:
    every kernel form the board admits against the emulator within EMU_BOUNDS, every stage.  The FC heads run at
    A = 1, 2, 16, 63, 65, 143, 144 outputs (slices with A mod 64 in {1, 63, 0})."""
    import torch
    import f16x3_model as M
    pkg = _pkg()
    E = pkg.engine
    planes = M.encode(M.positions(R, C, 37, 14))
    # a 1- or 2-cell board has a handful of positions: BatchNorm statistics from them would divide by ~sqrt(eps), so those
    # networks are calibrated on random planes
    cal = torch.rand((64, 5, R, C), generator=torch.Generator().manual_seed(6)) if R * C <= 2 else planes
    net = M.make_net("calibrated", R, C, ch, 2, seed=6, planes=cal).cuda().eval()
    planes = planes.cuda()
    ev = pkg.BatchedEvaluator(net)
    assert ev.mode == "f16x3"
    emu = M.emulate(M.Packed(net), planes)
    for nb, tb in _forms(R, C, ch):
        got = dict(tower=E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb),
                   feats=E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb, ev.g_hw, ev.g_hb))
        got["logits"], got["hidden"] = E.fc_heads(got["feats"], ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps)
        got["policy"], got["value"] = E.head_finish_f32(got["logits"], got["hidden"], ev.fc2_w, ev.fc2_b)
        e = M.errors(got, emu)
        print("%dx%d c%d form (%d, %d): %s" % (R, C, ch, nb, tb, _fmt(e)))
        bad = [(s, e[s], b) for s, b in M.EMU_BOUNDS["calibrated"].items() if not e[s] <= b]
        assert not bad, ((nb, tb), bad)
    p, v = ev(planes)
    assert torch.equal(p, got["policy"]) and torch.equal(v, got["value"])


def test_fc_heads_row_tile_switch():
    """csrc/yy_fc_heads.hip switches from 32-row to 64-row tiles above 2048 rows: at G = 2048 and 2049 (and 131) every row
    matches the emulator's FC stage within EMU_BOUNDS and the common rows are bit-identical across the three launches."""
    import torch
    import f16x3_model as M
    pkg = _pkg()
    E = pkg.engine
    net = M.make_net("calibrated", 8, 8, 64, 1, seed=8).cuda().eval()
    ev = pkg.BatchedEvaluator(net)
    pk = M.Packed(net)
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = torch.rand((2049, 2, 32 * 64), device="cuda", generator=g) * 3.0
    feats[feats < 1.2] = 0.0
    outs = {}
    for G in (131, 2048, 2049):
        f = feats[:G].contiguous()
        lg, hd = E.fc_heads(f, ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps)
        el, eh = M.emulate_fc(pk, f)
        e = (M.channel_error(lg, el, "logits"), M.channel_error(hd, eh, "hidden"))
        print("fc heads G=%d: logits %.2e hidden %.2e of the emulator" % (G, *e))
        assert e[0] <= M.EMU_BOUNDS["calibrated"]["logits"] and e[1] <= M.EMU_BOUNDS["calibrated"]["hidden"], (G, e)
        outs[G] = (lg, hd)
    for G in (131, 2048):
        assert torch.equal(outs[G][0], outs[2049][0][:G]) and torch.equal(outs[G][1], outs[2049][1][:G])


def test_f16x3_145_cells_falls_back_to_fp32():
    """A board of 145 cells (5 x 29) is past the split-f16 kernels: mode "auto" picks the float32 module, "f16x3" refuses."""
    import f16x3_model as M
    pkg = _pkg()
    net = M.make_net("calibrated", 5, 29, 32, 1, seed=9).cuda().eval()
    assert pkg.BatchedEvaluator(net).mode == "fp32"
    with pytest.raises(ValueError):
        pkg.BatchedEvaluator(net, "f16x3")


def _full(ev, planes, nb, tb, rows=None, n=None):
    E = _pkg().engine
    f = E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb, ev.g_hw, ev.g_hb, rows, n)
    lg, hd = E.fc_heads(f, ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps, n)
    return E.head_finish_f32(lg, hd, ev.fc2_w, ev.fc2_b, rows, n)


@pytest.mark.parametrize("R,C,ch", GEO_SHAPES + [(8, 8, 128), (6, 6, 128), (12, 12, 128)])
def test_nan_row_stays_in_its_row(R, C, ch):
    """Cross-board tracer: row k's planes set to NaN, k in {0, tb - 1, tb, G - 1} for every (column blocks, boards per
    workgroup) form of the board: every other row's policy and value are bit-identical to the clean run, every entry of row k
    is NaN -- dense, through a row gather, and through the evaluator's needs_eval compaction."""
    import torch
    import f16x3_model as M
    pkg = _pkg()
    E = pkg.engine
    net = M.make_net("calibrated", R, C, ch, 2, seed=10).cuda().eval()
    ev = pkg.BatchedEvaluator(net)
    forms = _forms(R, C, ch)
    G = 2 * max(tb for _, tb in forms) + 3
    clean = M.encode(M.positions(R, C, G, 15)).cuda()
    flags = torch.from_numpy((np.random.default_rng(5).random(G) < 0.6).astype(np.uint8)).cuda()
    rows, n = E.compact_rows(flags)
    p_ev, v_ev = ev(clean, needs_eval=flags)
    p_ev, v_ev = p_ev.clone(), v_ev.clone()
    for nb, tb in forms:
        p0, v0 = (t.clone() for t in _full(ev, clean, nb, tb))
        for k in sorted({0, tb - 1, tb, G - 1}):
            planes = clean.clone()
            planes[k] = float("nan")
            p, v = _full(ev, planes, nb, tb)
            other = torch.arange(G, device="cuda") != k
            assert bool(torch.isnan(p[k]).all()) and bool(torch.isnan(v[k])), ((nb, tb), k, p[k], v[k])
            assert torch.equal(p[other], p0[other]) and torch.equal(v[other], v0[other]), ((nb, tb), k)
            fl = flags.clone()
            fl[k] = 1
            rk, nk = E.compact_rows(fl)
            m = int(nk)
            pr, vr = _full(ev, planes, nb, tb, rk, nk)
            live = fl.bool()
            lo = live & other
            assert bool(torch.isnan(pr[k]).all()) and bool(torch.isnan(vr[k]))
            assert torch.equal(pr[lo], p0[lo]) and torch.equal(vr[lo], v0[lo]), ((nb, tb), k, m)
            pe, ve = ev(planes, needs_eval=fl)
            assert bool(torch.isnan(pe[k]).all()) and bool(torch.isnan(ve[k]))
            assert torch.equal(pe[lo], p0[lo]) and torch.equal(ve[lo], v0[lo]), ("evaluator", k)
    live = flags.bool()
    assert torch.equal(p_ev[live], p0[live]) and torch.equal(v_ev[live], v0[live])


def _overflow_eval(M, net, planes):
    ev = _pkg().BatchedEvaluator(net.cuda().eval())
    assert ev.mode == "f16x3"
    return ev(planes)


@pytest.mark.parametrize("how", ["scale", "nan"])
def test_overflow_rows_are_nan_exactly_there(how):
    """Overflow form (a): chosen rows' planes times 1e4 (activations far above 8190) or NaN.  Exactly those rows come out NaN
    in policy and value; every other row is bit-identical to the clean batch."""
    import torch
    import f16x3_model as M
    planes = M.encode(M.positions(8, 8, 40, 16)).cuda()
    net = M.make_net("calibrated", 8, 8, 128, 4, seed=11)
    p0, v0 = (t.clone() for t in _overflow_eval(M, net, planes))
    bad = [0, 5, 17, 39]
    p, v = _overflow_eval(M, net, M.poison_rows(planes, bad, how))
    mask = torch.zeros(40, dtype=torch.bool, device="cuda")
    mask[bad] = True
    print("form (a) %s: NaN rows policy %s value %s" % (how, torch.isnan(p).any(1).nonzero().flatten().tolist(),
                                                         torch.isnan(v).nonzero().flatten().tolist()))
    assert bool(torch.isnan(p[mask]).all()) and bool(torch.isnan(v[mask]).all())
    assert torch.equal(p[~mask], p0[~mask]) and torch.equal(v[~mask], v0[~mask])


@pytest.mark.parametrize("form", ["network", "value_head", "policy_head"])
def test_overflow_forms_poison_what_they_touch(form):
    """Overflow forms (b) a beta of 1e4 in the middle residual block: every policy and value NaN; (c) in the value head's
    BatchNorm: every value NaN, the policy bit-identical to the clean network's; (d) in the policy head's: every policy
    entry NaN, the value bit-identical."""
    import torch
    import f16x3_model as M
    planes = M.encode(M.positions(8, 8, 24, 17))
    pc = planes.cuda()
    clean = M.make_net("calibrated", 8, 8, 128, 4, seed=12, planes=planes)
    p0, v0 = (t.clone() for t in _overflow_eval(M, clean, pc))
    net = M.make_net("overflow", 8, 8, 128, 4, seed=12, planes=planes, form=form)
    ref = M.reference_f64(net, planes)
    where = {"network": ref["tower"], "value_head": ref["feats"][:, 1], "policy_head": ref["feats"][:, 0]}[form]
    assert float(where.max()) >= 8200.0
    p, v = _overflow_eval(M, net, pc)
    print("form %s: policy NaN %d of %d, value NaN %d of %d" % (form, int(torch.isnan(p).sum()), p.numel(),
                                                              int(torch.isnan(v).sum()), v.numel()))
    if form in ("network", "policy_head"):
        assert bool(torch.isnan(p).all())
    else:
        assert torch.equal(p, p0)
    if form in ("network", "value_head"):
        assert bool(torch.isnan(v).all())
    else:
        assert torch.equal(v, v0)


def test_overflow_boundary_is_8190():
    """One tower channel held at a constant activation A through the whole tower: A = 8000 and 8189 are represented exactly
    (the tower output holds A; policy within 2e-6 and value within 1e-5 of float64, measured 1.9e-7 / 2.0e-6); A = 8190 (x 2^3 = 65520, which rounds to float16
    infinity) and 8200 give NaN in every row."""
    import torch
    import f16x3_model as M
    pkg = _pkg()
    E = pkg.engine
    planes = M.encode(M.positions(8, 8, 16, 18))
    pc = planes.cuda()
    for A in (8000.0, 8189.0, 8190.0, 8200.0):
        net = M.make_net("boundary", 8, 8, 128, 4, seed=13, planes=planes, boundary=A).cuda().eval()
        ev = pkg.BatchedEvaluator(net)
        p, v = ev(pc)
        if A < M.F16_LIMIT:
            x = E.tower_g(pc, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, *ev.g_big)
            assert bool((x[:, 0] == A).all())
            ref = M.reference_f64(net, pc)
            ep, evv = float((p.double() - ref["policy"]).abs().max()), float((v.double() - ref["value"]).abs().max())
            print("activation %.0f: policy err %.2e value err %.2e" % (A, ep, evv))
            assert ep < 2e-6 and evv < 1e-5
        else:
            print("activation %.0f: policy NaN %d of %d, value NaN %d" % (A, int(torch.isnan(p).sum()), p.numel(), int(torch.isnan(v).sum())))
            assert bool(torch.isnan(p).all()) and bool(torch.isnan(v).all())


def test_overflowing_network_stops_the_search():
    """Form (b) (every evaluation NaN) through the searches: MCTS.search and one SelfPlayEngine move raise YYError instead of
    searching on finite, wrong numbers."""
    import torch
    import f16x3_model as M
    pkg = _pkg()
    game = pkg.YinYangGame(8, 8)
    net = M.make_net("overflow", 8, 8, 128, 4, seed=14, form="network").cuda().eval()
    ev = pkg.BatchedEvaluator(net)
    m = pkg.MCTS(game, ev, num_simulations=16, board_semantics="copied", dirichlet_noise=False)
    board = pkg.YinYangLogic(8, 8)
    with pytest.raises(pkg.YYError):
        m.search(board, 1)
    m.close()
    eng = pkg.SelfPlayEngine(game, ev, num_simulations=16, concurrent_games=8)
    eng.begin_run(8)
    with pytest.raises(pkg.YYError):
        eng.play_move()
    eng.close()
    torch.cuda.synchronize()
