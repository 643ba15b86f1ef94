"""CPU: the root Dirichlet noise of csrc/yy_selfplay.hip (k_root_noise) through its float64 restatement
(tests/philox_ref.root_noise), which tests/test_gpu_random_streams.py pins to the kernel element by element.

* the vectorised Philox4x32-10 against the scalar one and Random123's known answers;
* the law: two-sample Kolmogorov-Smirnov statistics against numpy's Generator.dirichlet for one rotating cell per row and
  for the sum over a fixed subset S of the legal cells (Beta(|S| a, (k - |S|) a)), and z-scores of the covariance of the
  cell pairs (a, a + 64) and (a, a + 128) against -1 / (k^2 (k a + 1)), at a in {0.03, 0.3, 1, 2.5} and k in {2, 16, 144,
  192} (k = 2 and 16 on cells 128...191 of 192 only);
* the structure: seeds s and s + 2^32, game ids g and g + 2^32, plies p and p + 1 give different, uncorrelated rows; for
  masks M1 in M2 the unnormalised cells agree;
* the power: each mutant of philox_ref.MUTANTS must fail one of those checks at the committed sizes and thresholds.

The seeds are fixed, so every statistic is deterministic.  Each comparison is held to a false-alarm probability of
P_CMP = 1e-6 / N_CMP (Bonferroni over N_CMP comparisons); the measured values are printed and listed in the docstrings.
"""
import math

import numpy as np
import pytest

from philox_ref import MUTANTS, draw, draw_np, philox4x32_10, philox4x32_10_np, root_noise

N_CMP = 200
P_CMP = 1e-6 / N_CMP
KS_LAMBDA = math.sqrt(math.log(2.0 / P_CMP) / 2.0)       # P(sqrt(n m / (n + m)) D > KS_LAMBDA) <= P_CMP (DKW, two-sample)


def _z_two_sided(p):
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
    return hi


Z_MAX = _z_two_sided(P_CMP)                                # 5.85
SUM_TOL = 1e-12
# numpy's dirichlet breaks sticks for alpha < 0.1 and returns 1 - (the others) for a component near 0, exactly 0 for ~8 % of
# the components at alpha = 0.03, k = 2; both samples are compared above this floor, where that cancellation is harmless
FLOOR = 1e-12

ALPHAS = (0.03, 0.3, 1.0, 2.5)
KS = (2, 16, 144, 192)


def ks2(a, b):
    """two-sample Kolmogorov-Smirnov statistic sqrt(n m / (n + m)) sup |F_a - F_b| (compare with KS_LAMBDA)"""
    a, b = np.sort(a), np.sort(b)
    z = np.concatenate([a, b])
    d = np.searchsorted(a, z, side="right") / len(a) - np.searchsorted(b, z, side="right") / len(b)
    return float(np.abs(d).max()) * math.sqrt(len(a) * len(b) / (len(a) + len(b)))


def cov_z(x, y, want):
    """z-score of the sample covariance of independent pairs (x, y) (known means) against want"""
    p = (x - x.mean()) * (y - y.mean())
    return abs(p.mean() - want) / (p.std() / math.sqrt(len(p)))


def corr_z(x, y):
    """sqrt(n) * Pearson correlation: ~N(0, 1) for independent samples"""
    return abs(float(np.corrcoef(x, y)[0, 1])) * math.sqrt(len(x))


def law_case(alpha, k):
    """(A, legal cells, rows): k = 2 and 16 on cells 128...191 of A = 192, k = 144 on a 12x12 board, k = 192 all of it"""
    cells = {2: np.array([130, 185]), 16: 128 + 4 * np.arange(16), 144: np.arange(144), 192: np.arange(192)}[k]
    A = 144 if k == 144 else 192
    n = {2: 40000, 16: 40000, 144: 3000, 192: 2500}[k]
    return A, cells, n


def law_stats(alpha, k, mutant=None):
    """{check name: (statistic, limit)} for the law of root_noise at (alpha, k)"""
    A, cells, n = law_case(alpha, k)
    i = ALPHAS.index(alpha) * len(KS) + KS.index(k)
    mask = np.zeros((n, A), np.uint8)
    mask[:, cells] = 1
    gid = 2 ** 33 + 977 * np.arange(n, dtype=np.int64)
    got = root_noise(2 ** 32 + 101 + i, gid, np.arange(n) % 7, np.ones(n, np.uint8), mask, alpha, mutant=mutant)
    ref = np.random.default_rng(500 + i).dirichlet([alpha] * k, n)
    x = got[:, cells]
    rot = np.arange(n) % k
    S = np.arange(0, k, 3)
    out = {
        "rows sum to 1": (float(np.abs(x.sum(1) - 1.0).max()), SUM_TOL),
        "KS marginal": (ks2(np.maximum(x[np.arange(n), rot], FLOOR), np.maximum(ref[np.arange(n), rot], FLOOR)), KS_LAMBDA),
        "KS subset sum": (ks2(np.maximum(x[:, S].sum(1), FLOOR), np.maximum(ref[:, S].sum(1), FLOOR)), KS_LAMBDA),
    }
    want = -1.0 / (k * k * (k * alpha + 1.0))
    for off in (64, 128):
        pairs = np.flatnonzero(np.isin(cells + off, cells))
        if pairs.size:
            a = pairs[np.arange(n) % pairs.size]
            b = np.searchsorted(cells, cells[a] + off)
            out["cov (a, a+%d)" % off] = (cov_z(x[np.arange(n), a], x[np.arange(n), b], want), Z_MAX)
    return out


def structure_stats(mutant=None):
    """{check name: (statistic, limit)}: the pairs (s, s + 2^32), (g, g + 2^32), (p, p + 1) give different, uncorrelated rows
    (sqrt(n) |corr| of one rotating cell per row); the rows of nested masks are proportional on the smaller one."""
    n, A, alpha = 1200, 192, 0.3
    mask = np.ones((n, A), np.uint8)
    on = np.ones(n, np.uint8)
    gid = 5 + 3 * np.arange(n, dtype=np.int64)
    ply = np.arange(n) % 301
    rot = (np.arange(n) * 7) % A
    base = root_noise(9, gid, ply, on, mask, alpha, mutant=mutant)
    out = {}
    for name, other in (("seed s + 2^32", root_noise(9 + 2 ** 32, gid, ply, on, mask, alpha, mutant=mutant)),
                        ("game g + 2^32", root_noise(9, gid + 2 ** 32, ply, on, mask, alpha, mutant=mutant)),
                        ("ply p + 1", root_noise(9, gid, ply + 1, on, mask, alpha, mutant=mutant))):
        same = int(sum(np.array_equal(base[r], other[r]) for r in range(n)))
        out[name + ": equal rows"] = (same, 0)
        out[name + ": corr"] = (corr_z(base[np.arange(n), rot], other[np.arange(n), rot]), Z_MAX)
    rng = np.random.default_rng(12)
    m2 = (rng.random((n, A)) < 0.6).astype(np.uint8)
    m1 = m2 * (rng.random((n, A)) < 0.5)
    m1[np.arange(n), np.argmax(m2, 1)] = 1                   # M1 in M2, never empty
    n1 = root_noise(9, gid, ply, on, m1, alpha, mutant=mutant)
    n2 = root_noise(9, gid, ply, on, m2, alpha, mutant=mutant)
    ratio = np.where(m1 != 0, n1 / np.where(m1 != 0, n2, 1.0), np.nan)
    spread = np.nanmax(ratio, 1) / np.nanmin(ratio, 1) - 1.0
    out["nested masks: ratio spread"] = (float(spread.max()), 1e-12)
    return out


def _failures(stats):
    return [(k, s, lim) for k, (s, lim) in stats.items() if not s <= lim]


def _fmt(stats):
    return "  ".join("%s %.3g/%.3g" % (k, s, lim) for k, (s, lim) in stats.items())


# ---- Philox
def test_vectorised_philox_equals_scalar_and_known_answers():
    """philox4x32_10_np against the scalar restatement on random words and on Random123's known-answer vectors; draw_np
    against draw on 64-bit seeds and game ids."""
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for c, k, want in kat:
        assert [int(w[0]) for w in philox4x32_10_np(*[[x] for x in c], [k[0]], [k[1]])] == want
    rng = np.random.default_rng(0)
    cs = rng.integers(0, 2 ** 32, size=(4, 300), dtype=np.uint64)
    ks = rng.integers(0, 2 ** 32, size=(2, 300), dtype=np.uint64)
    out = philox4x32_10_np(*cs, ks[0], ks[1])
    for i in range(300):
        assert [int(o[i]) for o in out] == philox4x32_10([int(c[i]) for c in cs], [int(ks[0][i]), int(ks[1][i])])
    games = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 63 - 1, -1], np.int64)
    for seed in (0, 7, 2 ** 32 + 7, 2 ** 64 - 1):
        for purpose in (0, 1, 2):
            got = draw_np(seed, games, np.arange(len(games)) * 50, purpose, np.arange(len(games)) * 64 + 63)
            for i, g in enumerate(games):
                assert [int(w[i]) for w in got] == draw(seed, int(g), i * 50, purpose, i * 64 + 63)


# ---- the law
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_root_noise_law(alpha, k):
    """Measured (KS_LAMBDA = 3.15, Z_MAX = 5.85; rows sum to 1 within 1.5e-15), for k = 2 / 16 / 144 / 192:
    alpha 0.03: KS marginal 1.35 / 1.10 / 0.62 / 0.62, KS subset 0.52 / 0.81 / 0.47 / 0.91;
    alpha 0.3:  KS marginal 0.68 / 0.94 / 1.14 / 1.27, KS subset 0.85 / 1.47 / 0.76 / 0.91;
    alpha 1:    KS marginal 1.31 / 0.85 / 1.01 / 1.16, KS subset 0.63 / 1.00 / 0.76 / 0.93;
    alpha 2.5:  KS marginal 1.13 / 0.68 / 0.89 / 1.34, KS subset 0.63 / 0.76 / 0.87 / 0.75;
    covariance z (a, a+64) and (a, a+128) at k = 144 and 192: at most 2.06 (alpha 0.03, k 192)."""
    stats = law_stats(alpha, k)
    print("\nalpha %g k %d: %s" % (alpha, k, _fmt(stats)))
    assert not _failures(stats)


def test_root_noise_structure():
    """Measured: no equal rows; sqrt(n) |corr| 2.59 (seed + 2^32), 1.26 (game + 2^32), 0.71 (ply + 1) against Z_MAX = 5.85;
    the ratio of nested-mask rows varies by at most 4.4e-16 on the smaller mask."""
    stats = structure_stats()
    print("\n" + _fmt(stats))
    assert not _failures(stats)


def test_small_alpha_rows_keep_their_noise():
    """alpha = 1e-3, k = 2: the linear total is below 2^-900 in 5 694 of 20 000 rows (measured); those go to log space, so
    every drawing row still sums to 1 and has a positive cell.  At alpha = 1 no row takes that path."""
    n = 20000
    mask = np.zeros((n, 192), np.uint8)
    mask[:, [3, 150]] = 1
    x, log_rows = root_noise(21, np.arange(n), np.zeros(n), np.ones(n), mask, 1e-3, with_log_rows=True)
    print("\nalpha 1e-3, k 2: %d of %d rows in log space" % (log_rows.sum(), n))
    assert 0.1 * n < log_rows.sum() < 0.9 * n
    assert np.abs(x.sum(1) - 1.0).max() <= SUM_TOL and (x.max(1) > 0).all()
    # alpha = 1: no boost, never in log space
    x1, log1 = root_noise(21, np.arange(n), np.zeros(n), np.ones(n), mask, 1.0, with_log_rows=True)
    assert not log1.any()


# ---- the power of the checks above
MUTANT_PLAN = {          # the checks to try first (every check runs if none of these fails)
    "no_boost": [("law", 0.3, 16)],
    "boost_alpha": [("law", 0.3, 16)],
    "u3_purpose0": [],
    "cell_mod64": [("law", 0.3, 144)],
    "seed_lo": [("structure",)],
    "d_half": [("law", 1.0, 16)],
    "norm_all": [("law", 0.3, 2)],
}


def _every_check():
    return [("structure",)] + [("law", a, k) for a in ALPHAS for k in KS]


@pytest.mark.parametrize("mutant", [pytest.param(m, marks=pytest.mark.xfail(strict=True, reason=(
    "u3 tied to u2 moves the gamma law by sup|dF| = 0.021 at a = 1, but the normalised marginal by far less: one-sample KS "
    "sqrt(n) D = 2.30 at n = 400 000 rows (0.78 unmutated), well under the limit"))) if m == "u3_purpose0" else m
    for m in MUTANTS])
def test_mutant_fails_a_check(mutant):
    """Each broken restatement must fail one of the checks above at the committed sizes and thresholds (the first failing
    one is printed); u3_purpose0 is out of reach of a CPU-sized sample and is a strict xfail.  Measured: no_boost and
    boost_alpha KS 47 / 45 (alpha 0.3, k 16), cell_mod64 covariance z 14.2 (alpha 0.3, k 144), seed_lo 1200 equal rows,
    d_half KS 5.24 (alpha 1, k 16), norm_all row sums off 1 by up to 1.0 (alpha 0.3, k 2)."""
    plan = MUTANT_PLAN[mutant]
    for check in plan + [c for c in _every_check() if c not in plan]:
        stats = structure_stats(mutant) if check[0] == "structure" else law_stats(check[1], check[2], mutant)
        bad = _failures(stats)
        if bad:
            print("\n%s fails %s: %s" % (mutant, check, ", ".join("%s %.3g > %.3g" % b for b in bad)))
            return
    pytest.fail("mutant %s passes every check" % mutant)
