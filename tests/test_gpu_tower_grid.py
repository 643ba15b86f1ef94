"""The 2x2 wave grid of the split-f16 tower (csrc/yy_tower_g.hip, k_tower_g22): the row-aligned 8-block form at 128 channels
(8x8, two boards per workgroup) with wave (mh, nh) owning 64 output channels x 4 column blocks.  Every output element keeps its
MFMA chain, so the kernel must write the bits of k_tower_g<4, 8, 9, true> (engine.tower_g(..., wave_grid=False)): head
features, tower activations, dense, gathered, gated, with overflowing activations and at the overflow boundary.  Its ReLU
(v_maximum3_f32) must equal relu_keep_nan on all 2^32 float32 inputs.  CPU checks read the compiled code: no scratch, the MFMA
count the convolution and skip structure predicts, half the LDS fragment reads per MFMA, no AGPR copies in the looped channel
group."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.normpath(os.path.join(HERE, "..", "yinyang-game-alphazero_amd", "csrc", "yy_tower_g.hip"))
OLD = "_ZN2tg9k_tower_gILi4ELi8ELi9ELb1E"
GRID = "_ZN2tg11k_tower_g22ILi3E"


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_bits_or_nan(a, b):
    """NaN in the same entries (a NaN's payload may differ), every other entry bit for bit."""
    import torch
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and _same_bits(a[~nan], b[~nan])


def _net(pkg, blocks=10, seed=5):
    import torch
    torch.manual_seed(seed)
    net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(8, 8), 128, blocks).cuda().eval()
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


def _planes(pkg, G, seed):
    import torch
    rng = np.random.default_rng(seed)
    return pkg.engine.encode_planes(torch.from_numpy(rng.integers(-1, 2, size=(G, 8, 8)).astype(np.int8)).cuda())


def _tower(ev, planes, grid, heads=True, rows=None, n=None, out=None, gate=(-1, 0x7FFFFFFF), form=(8, 2)):
    import yinyang_game_alphazero_amd as pkg
    hw, hb = (ev.g_hw, ev.g_hb) if heads else (None, None)
    return pkg.engine.tower_g(planes, ev.g_w, ev.g_b, ev.h3_layers, ev.g_exps, form[0], form[1], hw, hb, rows, n, out, gate,
                              wave_grid=grid)


def _policy_value(ev, planes, grid, rows=None, n=None):
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    f = _tower(ev, planes, grid, True, rows, n)
    lg, hd = E.fc_heads(f, ev.fc_w, ev.fc_b, ev.fc_jobs, ev.n_actions, ev.n_hidden, ev.fc_exps, n)
    return [t.clone() for t in E.head_finish_f32(lg, hd, ev.fc2_w, ev.fc2_b, rows, n)]


@pytest.mark.gpu
def test_wave_grid_writes_the_one_wave_per_slice_bits_dense_and_gathered():
    """Random 128 x 10 net: dense batches of odd and even sizes (a last workgroup with one live board included) and row
    gathers of odd counts; head features and tower activations of the 2x2 grid equal k_tower_g<4,8,9,true>'s bit for bit."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    ev = pkg.BatchedEvaluator(_net(pkg), "f16x3")
    assert ev.g_big == (8, 2)
    planes = _planes(pkg, 517, 13)
    for G in (1, 2, 3, 64, 255, 517):
        p = planes[:G].contiguous()
        for heads in (True, False):
            a, b = _tower(ev, p, True, heads), _tower(ev, p, False, heads)
            assert _same_bits(a, b), (G, heads)
            assert bool(torch.isfinite(a).all())
    for frac, seed in ((0.6, 3), (0.05, 4), (0.999, 5)):
        flags = torch.from_numpy((np.random.default_rng(seed).random(517) < frac).astype(np.uint8)).cuda()
        rows, n = E.compact_rows(flags)
        k = int(n)
        a, b = _tower(ev, planes, True, True, rows, n), _tower(ev, planes, False, True, rows, n)
        dense = _tower(ev, planes, True, True)
        assert _same_bits(a[:k], b[:k]) and _same_bits(a[:k], dense[rows[:k].long()]), (frac, k)


@pytest.mark.gpu
def test_wave_grid_through_the_gated_two_form_launch():
    """The evaluator's device-gated pair of launches (one-board form up to g_split live rows, the two-board form above it): for
    odd and boundary live row counts the rows written equal those of the pair with the one-wave-per-slice large form."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    ev = pkg.BatchedEvaluator(_net(pkg, seed=9), "f16x3")
    assert ev.g_small == (4, 1) and ev.g_big == (8, 2)
    S, G = ev.g_split, 1023
    planes = _planes(pkg, G, 4)
    rng = np.random.default_rng(6)
    for n_live in (1, S, S + 1, S + 2, (S + G) // 2 + 1, G):
        flags = torch.zeros(G, dtype=torch.uint8, device="cuda")
        flags[torch.from_numpy(rng.choice(G, n_live, replace=False)).cuda()] = 1
        rows, n = E.compact_rows(flags)
        got = []
        for grid in (True, False):
            out = torch.full((G, 2, 2048), -7.0, device="cuda")
            _tower(ev, planes, grid, True, rows, n, out, (-1, S), form=(4, 1))
            _tower(ev, planes, grid, True, rows, n, out, (S, 0x7FFFFFFF))
            got.append(out)
        assert _same_bits(got[0], got[1]), n_live


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["large", "wide", "saturated", "small3"])
def test_wave_grid_same_policy_and_value_across_regimes(regime):
    """tests/f16x3_model.py nets whose activations sit at the edges of the split-f16 range: (policy, value) through the 2x2 grid
    equal those through the one-wave-per-slice kernel, dense and gathered."""
    import torch
    import f16x3_model as M
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    planes = M.encode(M.positions(8, 8, 77, 31))
    net = M.make_net(regime, 8, 8, 128, 4, seed=17, planes=planes).cuda().eval()
    ev = pkg.BatchedEvaluator(net)
    assert ev.mode == "f16x3" and ev.g_big == (8, 2)
    pc = planes.cuda()
    a, b = _policy_value(ev, pc, True), _policy_value(ev, pc, False)
    for x, y in zip(a, b):
        assert _same_bits_or_nan(x, y), regime
    flags = torch.from_numpy((np.random.default_rng(2).random(77) < 0.5).astype(np.uint8)).cuda()
    rows, n = E.compact_rows(flags)
    live = flags.bool()
    ga, gb = _policy_value(ev, pc, True, rows, n), _policy_value(ev, pc, False, rows, n)
    for x, y in zip(ga, gb):
        assert _same_bits_or_nan(x[live], y[live]), regime


@pytest.mark.gpu
def test_wave_grid_keeps_the_overflow_rows_and_the_boundary():
    """Overflowing activations: rows scaled far past the format's top, NaN planes, networks whose value head or middle block
    overflows, and the 8189 / 8190 boundary.  NaN entries are the same entries in both kernels, every other entry has the same
    bits, and the overflow cases do produce NaN."""
    import torch
    import f16x3_model as M
    import yinyang_game_alphazero_amd as pkg
    planes = M.encode(M.positions(8, 8, 41, 16))
    pc = planes.cuda()
    cases = [(M.make_net("calibrated", 8, 8, 128, 4, seed=11), M.poison_rows(pc, [0, 1, 17, 40], "scale"), True),
             (M.make_net("calibrated", 8, 8, 128, 4, seed=11), M.poison_rows(pc, [3, 39], "nan"), True),
             (M.make_net("overflow", 8, 8, 128, 4, seed=12, planes=planes, form="value_head"), pc, True),
             (M.make_net("overflow", 8, 8, 128, 4, seed=12, planes=planes, form="network"), pc, True)]
    for A in (8189.0, 8190.0):
        cases.append((M.make_net("boundary", 8, 8, 128, 4, seed=13, planes=planes, boundary=A), pc, A >= 8190.0))
    for i, (net, x, overflows) in enumerate(cases):
        ev = pkg.BatchedEvaluator(net.cuda().eval())
        assert ev.mode == "f16x3"
        a, b = _policy_value(ev, x, True), _policy_value(ev, x, False)
        for u, v in zip(a, b):
            assert _same_bits_or_nan(u, v), i
        assert bool(torch.isnan(a[1]).any()) == overflows, i


@pytest.mark.gpu
def test_wave_grid_relu_equals_relu_keep_nan_on_every_float():
    """All 2^32 float32 bit patterns, in 16 launches: the one-VALU ReLU (v_maximum3_f32) has relu_keep_nan's bits for every
    input that is not a NaN (-0, subnormals and infinities included) and gives a NaN for every NaN."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    counts = torch.tensor([0, -1], dtype=torch.int32, device="cuda")      # [mismatches, smallest mismatching pattern]
    step = 1 << 28
    for start in range(0, 1 << 32, step):
        pkg.engine.tower_g_relu_check(start, step, counts)
    c = counts.cpu().numpy().view(np.uint32)
    assert c[0] == 0, "ReLU differs on %d inputs, first 0x%08x" % (c[0], c[1])


def _body(lines, name):
    start = next(i for i, l in enumerate(lines) if l.startswith(name) and l.split()[0].endswith(":"))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1]


def _count(body, prefix):
    return sum(1 for l in body if l.strip().startswith(prefix))


def _loops(body):
    """Instruction ranges of the kernel's loops (a label and the branch back to it) that issue MFMAs."""
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if re.match(r"^\.LBB\S+:", l)}
    out = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\S+)", l)
        if m and labels.get(m.group(1), i) < i:
            seg = body[labels[m.group(1)]:i + 1]
            if _count(seg, "v_mfma"):
                out.append(seg)
    return out


def test_wave_grid_kernel_code():
    """CPU: compile csrc/yy_tower_g.hip for gfx950 and read the assembly of k_tower_g22<3>.
    * No private segment (no spill) and no scratch instruction.
    * v_mfma count: two compiled copies (one per wave column half), each the stem, the peeled and the looped channel group of a
      body layer at 9 taps x 4 blocks x 12 MFMAs less the 3 dropped (tap, block) pairs, plus the 1x1 heads (8 blocks x 4 k-steps
      x 3) once.
    * ds_read_b128 per MFMA at least 1.8 times fewer than k_tower_g<4,8,9,true>.
    * The looped channel group (the innermost loop that issues 396 MFMAs, one per copy) has no v_accvgpr_read / write and no
      non-MFMA VALU beyond one address add per LDS fragment and one 64-bit weight address per four weight loads."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                               "--cuda-device-only", "-S", "-o", os.path.join(tmp, "tg.s"), SRC], cwd=tmp)
        asm = open(os.path.join(tmp, "tg.s")).read()
    lines = asm.splitlines()
    grid, old = _body(lines, GRID), _body(lines, OLD)
    seg = re.search(re.escape(GRID) + r"[^\n]*\.private_seg_size, (\d+)", asm)
    assert int(seg.group(1)) == 0
    assert _count(grid, "scratch_") == 0
    per_group = (9 * 4 - 3) * 12
    n_mfma = _count(grid, "v_mfma")
    print("v_mfma: grid %d (per copy and channel group %d), one wave per slice %d" % (n_mfma, per_group, _count(old, "v_mfma")))
    assert n_mfma == 2 * 3 * per_group + 8 * 4 * 3
    r_grid = _count(grid, "ds_read_b128") / n_mfma
    r_old = _count(old, "ds_read_b128") / _count(old, "v_mfma")
    print("ds_read_b128 per MFMA: grid %.4f, one wave per slice %.4f (%.2fx)" % (r_grid, r_old, r_old / r_grid))
    assert r_old >= 1.8 * r_grid
    inner = [s for s in _loops(grid) if _count(s, "v_mfma") == per_group]
    assert len(inner) == 2
    for s in inner:
        assert _count(s, "v_accvgpr_read") == 0 and _count(s, "v_accvgpr_write") == 0
        valu = [l.split()[0] for l in s if l.strip().startswith("v_") and not l.strip().startswith("v_mfma")]
        n_frag = _count(s, "ds_read_b128") // 2
        n_wload = _count(s, "global_load_dwordx4")
        assert len(valu) <= n_frag + n_wload // 4, sorted(set(valu))
        assert set(valu) <= {"v_add_u32_e32", "v_lshl_add_u64"}, sorted(set(valu))
