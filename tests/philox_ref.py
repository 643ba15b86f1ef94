"""Host restatement (test helper) of the counter-based streams of csrc/yy_selfplay.hip: Philox4x32-10 keyed by the seed with
counter (game lo, game hi, ply << 8 | purpose, element), and the move choice built on it (self_play.py:143-160)."""
import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c = [int(x) & M32 for x in counter]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def draw(seed, game, ply, purpose, element):
    game &= 0xFFFFFFFFFFFFFFFF
    return philox4x32_10([game & M32, game >> 32, ((ply << 8) | purpose) & M32, element], [seed & M32, (seed >> 32) & M32])


def u01(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def sample_action(seed, game, ply, pi, mask, thr):
    """pi float64 [A], mask {0,1} [A] -> action, the same float64 operations in the same order as k_sample_actions."""
    r = draw(seed, game, ply, 1, 0)
    u = u01(r[0], r[1])
    A = len(pi)
    pick = -1
    if ply < thr:
        tot, legal = 0.0, 0
        for a in range(A):
            tot += float(pi[a]) if mask[a] else 0.0
            legal += 1 if mask[a] else 0
        if tot > 0.0:
            target, c = u * tot, 0.0
            for a in range(A):
                w = float(pi[a]) if mask[a] else 0.0
                c += w
                if w > 0.0:
                    pick = a
                    if c > target:
                        break
        elif legal > 0:
            k = min(int(u * legal), legal - 1)
            for a in range(A):
                if mask[a]:
                    if k == 0:
                        pick = a
                        break
                    k -= 1
    else:
        mx = float(np.max(pi))
        best = [a for a in range(A) if float(pi[a]) == mx]
        pick = best[min(int(u * len(best)), len(best) - 1)]
    return pick


# ---- vectorised streams and the root Dirichlet noise (k_root_noise)
def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """philox4x32_10 over numpy arrays (any broadcastable mix of arrays and ints < 2^32): the four output words as uint64."""
    c = [np.asarray(x, np.uint64) & np.uint64(M32) for x in (c0, c1, c2, c3)]
    k0, k1 = np.asarray(k0, np.uint64) & np.uint64(M32), np.asarray(k1, np.uint64) & np.uint64(M32)
    m, s = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & m, (p0 >> s) ^ c[3] ^ k1, p0 & m]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c


def draw_np(seed, game, ply, purpose, element, mutant=None):
    """draw() over arrays of games (int64, read as uint64), plies and elements; the seed is one int."""
    game = np.asarray(game, np.int64).view(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k1 = 0 if mutant == "seed_lo" else seed >> 32
    ctr = (np.asarray(ply, np.uint64) << np.uint64(8)) | np.uint64(purpose)
    return philox4x32_10_np(game & np.uint64(M32), game >> np.uint64(32), ctr, element, seed & M32, k1)


def u01_np(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


LOG_SPACE_BELOW = 2.0 ** -900     # k_root_noise redoes a drawing row in log space when its linear total is below this
MUTANTS = ("no_boost", "boost_alpha", "u3_purpose0", "cell_mod64", "seed_lo", "d_half", "norm_all")


def gamma_draw(seed, game, ply, cell, alpha, mutant=None):
    """gamma_draw of yy_selfplay.hip for arrays of (game, ply, cell): Marsaglia-Tsang on a = alpha (+1 when alpha < 1), attempt t
    of a cell on element cell * 64 + t; returns (g, ub) with g = d after 64 rejections.  The cell's value is g * ub^(1/alpha)
    when alpha < 1 (the boost), else g.

    mutant (tests/test_random_streams.py breaks the law on purpose): "u3_purpose0" takes u3 from the purpose-0 word (r.z, r.w)
    that gave u2, "cell_mod64" draws cell a on the counter of a % 64, "seed_lo" drops the seed's high word, "d_half" uses
    d = a - 1/2; the others act in root_noise."""
    game, ply, cell = (np.asarray(x) for x in (game, ply, cell))
    boost = alpha < 1.0
    a = alpha + 1.0 if boost else alpha
    d = a - (0.5 if mutant == "d_half" else 1.0 / 3.0)
    c = 1.0 / np.sqrt(9.0 * d)
    ecell = (cell % 64 if mutant == "cell_mod64" else cell).astype(np.uint64)
    g = np.full(cell.shape, d)
    ub = np.full(cell.shape, 0.5)
    todo = np.arange(cell.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(64):
            if todo.size == 0:
                break
            el = ecell.ravel()[todo] * np.uint64(64) + np.uint64(t)
            gm, pl = game.ravel()[todo], ply.ravel()[todo]
            r = draw_np(seed, gm, pl, 0, el, mutant)
            q = draw_np(seed, gm, pl, 2, el, mutant)
            u1, u2 = 1.0 - u01_np(r[0], r[1]), u01_np(r[2], r[3])
            z = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
            v1 = 1.0 + c * z
            v = v1 * v1 * v1
            u3 = 1.0 - (u01_np(r[2], r[3]) if mutant == "u3_purpose0" else u01_np(q[0], q[1]))
            acc = (v1 > 0.0) & (np.log(u3) < 0.5 * z * z + d - d * v + d * np.log(v))
            hit = todo[acc]
            g.ravel()[hit] = d * v[acc]
            ub.ravel()[hit] = 1.0 - u01_np(q[2], q[3])[acc]
            todo = todo[~acc]
    return g, ub


def _wave_sum(x3):
    """[G, 192] -> [G]: each lane's cells lane, lane + 64, lane + 128 summed in that order, then the xor butterfly 32 ... 1."""
    v = (x3[:, 0:64] + x3[:, 64:128]) + x3[:, 128:192]
    for o in (32, 16, 8, 4, 2, 1):
        w = v.reshape(len(v), 32 // o, 2, o)         # lane l's partner l ^ o: the other half of its block of 2 * o lanes
        v = (w + w[:, :, ::-1, :]).reshape(len(v), 64)
    return v[:, 0]


def root_noise(seed, game_id, ply, draw, mask, alpha, mutant=None, with_log_rows=False):
    """k_root_noise operation for operation: float64 [G, A] Dirichlet(alpha) noise over the legal cells (mask != 0) of the rows
    with draw != 0, zero rows elsewhere and where the total is 0.  A drawing row whose linear total is below 2^-900 (exactly 0
    included) is redone in log space: log x = log g + log(ub) / alpha, minus the row maximum, exp, normalised in the same
    order.  with_log_rows also returns the bool [G] of rows that took that path.

    mutant: see gamma_draw; "no_boost" drops the boost, "boost_alpha" boosts by ub^alpha, "norm_all" normalises over all A
    cells instead of the legal ones."""
    mask = np.asarray(mask) != 0
    G, A = mask.shape
    assert 1 <= A <= 192 and 0 < alpha < np.inf
    on = np.asarray(draw) != 0
    live = (mask | (mutant == "norm_all")) & on[:, None]
    rows, cells = np.nonzero(live)
    gid = np.asarray(game_id, np.int64)[rows]
    pl = np.asarray(ply, np.int64)[rows]
    g, ub = gamma_draw(seed, gid, pl, cells, alpha, mutant)
    boost = alpha < 1.0 and mutant != "no_boost"
    with np.errstate(divide="ignore", under="ignore"):
        x = g * np.power(ub, alpha if mutant == "boost_alpha" else 1.0 / alpha) if boost else g
        lx = np.log(g) + np.log(ub) / alpha if boost else np.log(g)
    X = np.zeros((G, 192))
    X[rows, cells] = x
    tot = _wave_sum(X)
    legal = np.zeros((G, 192), bool)
    legal[:, :A] = mask & on[:, None]
    out = np.where(legal & (tot > 0.0)[:, None], X / np.where(tot > 0.0, tot, 1.0)[:, None], 0.0)
    L = np.full((G, 192), -np.inf)
    L[rows, cells] = lx
    L = np.where(legal, L, -np.inf)
    m = L.max(1)
    redo = on & (tot < LOG_SPACE_BELOW) & (m > -np.inf)
    if redo.any():
        with np.errstate(under="ignore", invalid="ignore"):
            E = np.where(legal[redo], np.exp(L[redo] - m[redo, None]), 0.0)
        out[redo] = E / _wave_sum(E)[:, None]
    out = out[:, :A]
    return (out, redo) if with_log_rows else out
