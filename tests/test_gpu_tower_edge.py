"""Layer edges of the 2x2 wave grid of the split-f16 tower (csrc/yy_tower_g.hip, k_tower_g22): a lane owns 8 consecutive output
channels per M-block pair (load_w22 fetches its A rows accordingly) and stores them as one 16-byte piece per part.  Which
channel a row of an M block stands for enters no MFMA chain, so the kernel must still write the bits of k_tower_g on the
one-wave-per-slice grid (wave_grid=False) and in the column layout (column_layout=True); a wrong row permutation moves whole
channels, so the bound is equality.  Shapes are the smallest that can go wrong: one to three rows (an odd count leaves a padding
board in the last workgroup), depths 1 (stem only), 3 (a KEEP layer, then a CONV2 layer), 5 and 21 (full depth)."""
import numpy as np
import pytest

LAYERS = (1, 3, 5, 21)
POOL = 7          # planes a compacted launch gathers its rows from


@pytest.fixture(scope="module")
def tower():
    """One random 128 x 10 network (batch-norm statistics randomised), packed once, and POOL random positions.  A shallower
    tower is a prefix of the weight stream ([layer][channel group][tap]) and of the bias rows."""
    import torch
    import yinyang_game_alphazero_amd as pkg
    torch.manual_seed(23)
    net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(8, 8), 128, 10).cuda().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.7, 1.3)
                m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_(0, 0.05)
    ev = pkg.BatchedEvaluator(net, "f16x3")
    assert ev.g_big == (8, 2) and ev.h3_layers == 21 and ev.g_b.shape == (21, 128)
    rng = np.random.default_rng(29)
    planes = pkg.engine.encode_planes(torch.from_numpy(rng.integers(-1, 2, size=(POOL, 8, 8)).astype(np.int8)).cuda())
    return ev, planes


def _run(ev, planes, n_layers, heads, rows=None, n=None, **form):
    import yinyang_game_alphazero_amd as pkg
    w = ev.g_w[:9 + 36 * (n_layers - 1)]
    hw, hb = (ev.g_hw, ev.g_hb) if heads else (None, None)
    return pkg.engine.tower_g(planes, w, ev.g_b[:n_layers], n_layers, ev.g_exps, 8, 2, hw, hb, rows, n, **form).contiguous()


def _equal(a, b):
    """torch.equal on the bit patterns (so that -0 and +0 differ)"""
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _shuffled_rows(k, seed):
    import torch
    rows = np.zeros(POOL, np.int32)
    rows[:k] = np.random.default_rng(seed).permutation(POOL)[:k]
    return torch.from_numpy(rows).cuda(), torch.tensor([k], dtype=torch.int32, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("n_layers", LAYERS)
def test_edge_stores_keep_every_bit(tower, n_layers):
    """Dense launches of 1, 2 and 3 rows and compacted launches of 1, 2 and 3 shuffled rows out of 7: head features and tower
    activations of the default (2x2 grid) call equal those of wave_grid=False and of column_layout=True."""
    import torch
    ev, planes = tower
    for G in (1, 2, 3):
        for heads in (True, False):
            p = planes[:G].contiguous()
            a = _run(ev, p, n_layers, heads)
            assert bool(torch.isfinite(a).all()) and bool((a != 0).any()), (G, heads)
            assert _equal(a, _run(ev, p, n_layers, heads, wave_grid=False)), ("dense", G, heads)
            assert _equal(a, _run(ev, p, n_layers, heads, column_layout=True)), ("dense", G, heads)
            rows, n = _shuffled_rows(G, 31 + G)
            c = _run(ev, planes, n_layers, heads, rows, n)[:G]
            assert bool(torch.isfinite(c).all()), (G, heads)
            assert _equal(c, _run(ev, planes, n_layers, heads, rows, n, wave_grid=False)[:G]), ("compacted", G, heads)
            assert _equal(c, _run(ev, planes, n_layers, heads, rows, n, column_layout=True)[:G]), ("compacted", G, heads)
            # the gathered rows are the rows themselves: row i of the compacted launch is planes[rows[i]] evaluated densely
            assert _equal(c, _run(ev, planes, n_layers, heads)[rows[:G].long()]), ("gather", G, heads)


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [True, False])
def test_edge_stores_keep_a_nan_in_its_row(tower, heads):
    """One NaN in one plane of the middle row of three (it shares its workgroup with row 0), full depth: every output of that
    row is NaN (21 3x3 layers reach every cell and channel), rows 0 and 2 keep the bits of the clean run, and the
    one-wave-per-slice kernel has NaN in the same entries."""
    import torch
    ev, planes = tower
    clean = planes[:3].contiguous()
    bad = clean.clone()
    bad[1, 2, 3, 4] = float("nan")
    a, b = _run(ev, clean, 21, heads), _run(ev, bad, 21, heads)
    assert bool(torch.isnan(b[1]).all())
    assert bool(torch.isfinite(a).all())
    assert _equal(b[0], a[0]) and _equal(b[2], a[2])
    r = _run(ev, bad, 21, heads, wave_grid=False)
    assert torch.equal(torch.isnan(b), torch.isnan(r)) and _equal(b[0], r[0]) and _equal(b[2], r[2])
