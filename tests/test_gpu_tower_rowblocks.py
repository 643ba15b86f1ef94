"""The row-aligned column blocks of the split-f16 tower (csrc/yy_tower_g.hip, RB forms): where boards * C == 16 and the form
has R column blocks (8x8 with two boards per workgroup, 4x4 with four), block r holds row r of every board and the kernel drops
the MFMAs of the (tap, block) pairs that only read the zero border.  Those MFMAs only added exact zeros, so the row-aligned
kernel must write the bits the column layout writes (engine.tower_g(..., column_layout=True)): head features, tower
activations, (policy, value), dense, gathered, gated, and with overflowing activations.  One CPU check reads the compiled
code: 1/12 of the tower's MFMAs are gone at 8x8, and no register spill was added."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.normpath(os.path.join(HERE, "..", "yinyang-game-alphazero_amd", "csrc", "yy_tower_g.hip"))


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _net(pkg, R, C, blocks=10, seed=5):
    import torch
    torch.manual_seed(seed)
    net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(R, C), 128, blocks).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.7, 1.3)
                m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_(0, 0.05)
    return net


def _planes(pkg, R, C, G, seed):
    import torch
    rng = np.random.default_rng(seed)
    return pkg.engine.encode_planes(torch.from_numpy(rng.integers(-1, 2, size=(G, R, C)).astype(np.int8)).cuda())


def _engine():
    import yinyang_game_alphazero_amd as pkg
    return pkg.engine


def _both(ev, planes, nb, tb, heads, rows=None, n=None):
    """(row-aligned, column layout) outputs of one tower launch: head features, or the tower activations."""
    E = _engine()
    hw, hb = (ev.g_hw, ev.g_hb) if heads else (None, None)
    return [E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb, hw, hb, rows, n, column_layout=cl) for cl in (False, True)]


def _policy_value(ev, planes, column_layout, rows=None, n=None):
    """The evaluator's (policy, value) with the large form's tower in the chosen layout."""
    E = _engine()
    nb, tb = ev.g_big
    f = E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, nb, tb, ev.g_hw, ev.g_hb, rows, n, column_layout=column_layout)
    lg, hd = E.fc_heads(f, ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps, n)
    return E.head_finish_f32(lg, hd, ev.fc2_w, ev.fc2_b, rows, n)


@pytest.mark.gpu
@pytest.mark.parametrize("R,nb,tb", [(8, 8, 2), (4, 4, 4)])
def test_row_aligned_blocks_write_the_column_layout_bits(R, nb, tb):
    """Dense batches whose last workgroup holds every possible number of live boards (a single one included), then a row
    gather: head features and tower activations of the row-aligned kernel equal the column layout's, bit for bit."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    net = _net(pkg, R, R)
    ev = pkg.BatchedEvaluator(net, "f16x3")
    if R == 8:
        assert ev.g_big == (nb, tb)
    planes = _planes(pkg, R, R, 4 * tb * 16 + 1, 13)
    for G in sorted({1, 2, tb - 1, tb, tb + 1, 2 * tb - 1, planes.shape[0]} - {0}):
        p = planes[:G].contiguous()
        for heads in (True, False):
            rb, col = _both(ev, p, nb, tb, heads)
            assert _same_bits(rb, col), (G, heads)
            assert bool(torch.isfinite(rb).all())
    G = planes.shape[0]
    flags = torch.from_numpy((np.random.default_rng(3).random(G) < 0.6).astype(np.uint8)).cuda()
    rows, n = E.compact_rows(flags)
    k = int(n)
    dense, _ = _both(ev, planes, nb, tb, True)
    rb, col = _both(ev, planes, nb, tb, True, rows, n)
    assert _same_bits(rb[:k], col[:k]) and _same_bits(rb[:k], dense[rows[:k].long()])


@pytest.mark.gpu
def test_row_aligned_blocks_give_the_same_policy_and_value():
    """8x8, 128 x 10: the evaluator's (policy, value) from the row-aligned tower equal those from the column layout, dense and
    through the row compaction, and equal what BatchedEvaluator itself returns."""
    import yinyang_game_alphazero_amd as pkg
    import torch
    E = pkg.engine
    ev = pkg.BatchedEvaluator(_net(pkg, 8, 8, seed=7), "f16x3")
    planes = _planes(pkg, 8, 8, 301, 21)
    p_rb, v_rb = (t.clone() for t in _policy_value(ev, planes, False))
    p_col, v_col = _policy_value(ev, planes, True)
    assert _same_bits(p_rb, p_col) and _same_bits(v_rb, v_col)
    p_ev, v_ev = ev(planes)
    assert _same_bits(p_ev, p_rb) and _same_bits(v_ev, v_rb)
    flags = torch.from_numpy((np.random.default_rng(8).random(301) < 0.5).astype(np.uint8)).cuda()
    rows, n = E.compact_rows(flags)
    pr, vr = (t.clone() for t in _policy_value(ev, planes, False, rows, n))     # written back to the rows' own positions
    pc, vc = _policy_value(ev, planes, True, rows, n)
    live = flags.bool()
    assert _same_bits(pr[live], pc[live]) and _same_bits(vr[live], vc[live])
    assert _same_bits(pr[live], p_rb[live]) and _same_bits(vr[live], v_rb[live])


@pytest.mark.gpu
def test_row_aligned_blocks_through_the_gated_two_form_launch():
    """The evaluator's device-gated pair of launches (one board per workgroup up to g_split live rows, the row-aligned two-board
    form above it): for live row counts on both sides of the split, the rows written equal the column layout's pair."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    ev = pkg.BatchedEvaluator(_net(pkg, 8, 8, seed=9), "f16x3")
    assert ev.g_small == (4, 1) and ev.g_big == (8, 2)
    S, G = ev.g_split, 1024
    planes = _planes(pkg, 8, 8, G, 4)
    rng = np.random.default_rng(6)
    for n_live in (1, S, S + 1, (S + G) // 2 + 1, G):
        flags = torch.zeros(G, dtype=torch.uint8, device="cuda")
        flags[torch.from_numpy(rng.choice(G, n_live, replace=False)).cuda()] = 1
        rows, n = E.compact_rows(flags)
        got = []
        for cl in (False, True):
            out = torch.full((G, 2, 2048), -7.0, device="cuda")
            E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, 4, 1, ev.g_hw, ev.g_hb, rows, n, out, (-1, S), column_layout=cl)
            E.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, 8, 2, ev.g_hw, ev.g_hb, rows, n, out, (S, 0x7FFFFFFF),
                      column_layout=cl)
            got.append(out)
        assert _same_bits(got[0], got[1]), n_live


@pytest.mark.gpu
def test_row_aligned_blocks_keep_the_overflow_rows():
    """Overflowing activations (tests/f16x3_model.py): rows whose planes are scaled far past the format's top and a network
    whose middle block overflows.  The NaN entries of (policy, value) are the same entries in both layouts and every other
    entry has the same bits."""
    import torch
    import f16x3_model as M
    import yinyang_game_alphazero_amd as pkg
    planes = M.encode(M.positions(8, 8, 41, 16))
    pc = planes.cuda()
    cases = [(M.make_net("calibrated", 8, 8, 128, 4, seed=11), M.poison_rows(pc, [0, 1, 17, 40], "scale")),
             (M.make_net("overflow", 8, 8, 128, 4, seed=12, planes=planes, form="value_head"), pc),
             (M.make_net("overflow", 8, 8, 128, 4, seed=12, planes=planes, form="network"), pc)]
    for i, (net, x) in enumerate(cases):
        ev = pkg.BatchedEvaluator(net.cuda().eval())
        assert ev.mode == "f16x3"
        rb = [t.clone() for t in _policy_value(ev, x, False)]
        col = _policy_value(ev, x, True)
        for a, b in zip(rb, col):
            nan = torch.isnan(a)
            assert torch.equal(nan, torch.isnan(b)), i
            assert _same_bits(a[~nan], b[~nan]), i
        assert bool(torch.isnan(rb[1]).any()), i


def _kernel_stats(asm, name):
    """(v_mfma count, private segment bytes) of the kernel whose mangled name starts with `name` in a .s file."""
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(name) and l.split()[0].endswith(":"))
    n = 0
    for l in lines[start:]:
        if "v_mfma" in l:
            n += 1
        if "s_endpgm" in l:
            break
    seg = re.search(re.escape(name) + r"[^\n]*\.private_seg_size, (\d+)", asm)
    return n, int(seg.group(1))


def test_row_aligned_kernel_drops_a_twelfth_of_the_tower_mfmas():
    """CPU: compile csrc/yy_tower_g.hip for gfx950 and read the assembly.  At 128 channels and 8 column blocks the row-aligned
    kernel has 3 * 36 fewer v_mfma instructions than the column kernel (the stem, and the peeled first and looped channel
    groups of a body layer, each lose 6 of 72 (tap, block) pairs of 6 MFMAs): 1/12 of the convolutions' MFMAs, the 1x1 head
    MFMAs (8 blocks x 4 k-steps x 3) unchanged.  Its private segment (register spills) is no larger than the column kernel's."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                               "--cuda-device-only", "-S", "-o", os.path.join(tmp, "tg.s"), SRC], cwd=tmp)
        asm = open(os.path.join(tmp, "tg.s")).read()
    col_n, col_seg = _kernel_stats(asm, "_ZN2tg9k_tower_gILi4ELi8ELi9ELb0E")
    rb_n, rb_seg = _kernel_stats(asm, "_ZN2tg9k_tower_gILi4ELi8ELi9ELb1E")
    head = 8 * 4 * 3
    print("v_mfma: column layout %d, row-aligned %d; private segment %d / %d bytes" % (col_n, rb_n, col_seg, rb_seg))
    assert col_n - rb_n == 3 * 36
    assert (col_n - rb_n) * 12 == col_n - head
    assert rb_seg <= col_seg
    n4, _ = _kernel_stats(asm, "_ZN2tg9k_tower_gILi4ELi4ELi9ELb0E")
    r4, _ = _kernel_stats(asm, "_ZN2tg9k_tower_gILi4ELi4ELi9ELb1E")
    assert n4 - r4 == 3 * 36
