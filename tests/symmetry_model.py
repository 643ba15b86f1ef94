"""Host restatement (test helper) of symmetry-randomised evaluation (include/yy_engine.h, YY_FLAG_EVAL_SYMMETRY): the draw
s = sym(seed, position) on tests/philox_ref.py, the board transforms T_s in numpy's own words, the cell map T_s(a), and the
host-wrapped evaluator that is the feature's exact reference: an engine with the option OFF driven by wrap(inner) must equal
an engine with the option ON driven by the bare inner evaluator, bit for bit."""
import numpy as np

from philox_ref import M32, philox4x32_10_np

SYM_TAG = 0x59595F53594D5F34      # the domain tag in the key: every other stream keys with the seed itself


DRAW_SEED = 2024                   # the seed of the draw tests; test_evaluation_symmetry_host.py checks the spread it gives
DRAW_SHAPES = ((4, 4), (5, 7), (9, 12), (12, 12))


def group_size(R, C):
    return 8 if R == C else 4


def positions(shape, n=512):
    """n distinct random positions int8 [n,R,C] (cells uniform over empty / black / white), the same on every call."""
    rng = np.random.RandomState(1000 * shape[0] + shape[1])
    boards = np.unique(rng.randint(-1, 2, size=(2 * n,) + tuple(shape)).astype(np.int8), axis=0)
    assert len(boards) >= n
    return np.ascontiguousarray(boards[rng.permutation(len(boards))[:n]])


def pack_words(boards):
    """int8 [G,R,C] -> (black, white) uint64 [G,NW]: bit a of the words = cell a = r*C + c."""
    flat = np.asarray(boards, np.int8).reshape(len(boards), -1)
    G, A = flat.shape
    nw = (A + 63) // 64
    out = []
    for colour in (1, -1):
        w = np.zeros((G, nw), np.uint64)
        for a in range(A):
            w[:, a >> 6] |= (flat[:, a] == colour).astype(np.uint64) << np.uint64(a & 63)
        out.append(w)
    return out


def draw(boards, seed):
    """s for every board of int8 [G,R,C]: Philox4x32-10 keyed by seed ^ SYM_TAG, the NW word pairs chained -- block i has the
    counter (black[i] lo, black[i] hi, white[i] lo, white[i] hi) ^ the output of block i - 1 (zero for i = 0) -- and s = the top
    3 (square boards) or 2 bits of the last block's first word."""
    boards = np.asarray(boards, np.int8)
    G, R, C = boards.shape
    black, white = pack_words(boards)
    key = (int(seed) & 0xFFFFFFFFFFFFFFFF) ^ SYM_TAG
    m, s32 = np.uint64(M32), np.uint64(32)
    h = [np.zeros(G, np.uint64) for _ in range(4)]
    for i in range(black.shape[1]):
        c = [h[0] ^ (black[:, i] & m), h[1] ^ (black[:, i] >> s32), h[2] ^ (white[:, i] & m), h[3] ^ (white[:, i] >> s32)]
        h = philox4x32_10_np(c[0], c[1], c[2], c[3], key & M32, key >> 32)
    return (h[0] >> np.uint64(29 if R == C else 30)).astype(np.int8)


def transform(board, s):
    """T_s of one board [R,C] (any dtype), in numpy's words."""
    board = np.asarray(board)
    R, C = board.shape
    if R == C:
        out = np.rot90(board, s & 3)
        return np.fliplr(out) if s & 4 else out
    out = np.flipud(board) if s & 1 else board
    return np.fliplr(out) if s & 2 else out


def inverse(board, s):
    """T_s^-1 of one board."""
    board = np.asarray(board)
    R, C = board.shape
    if R == C:
        out = np.fliplr(board) if s & 4 else board
        return np.rot90(out, -(s & 3))
    return transform(board, s)          # two commuting flips


def cell_map(R, C, s):
    """T_s(a) for every cell a: int64 [A], where cell a lands.  Derived from transform() itself: the transformed index board
    holds at every destination the cell that landed there."""
    landed = transform(np.arange(R * C).reshape(R, C), s).reshape(-1)
    out = np.empty(R * C, np.int64)
    out[landed] = np.arange(R * C)
    return out


def transform_boards(boards, s):
    return np.stack([np.ascontiguousarray(transform(b, int(k))) for b, k in zip(boards, s)]) if len(boards) else np.asarray(boards)


class Wrapped:
    """inner evaluator -> the evaluator an option-off engine must be driven with to play the option-on engine's games:
    planes of original positions -> board -> s -> T_s(board) -> encode -> inner -> policy[a] = row[T_s(a)], value as is."""

    def __init__(self, pkg, inner, seed, row_independent=True):
        self.pkg, self.inner, self.seed, self.row_independent = pkg, inner, seed, row_independent

    def __call__(self, planes):
        import torch
        boards = (planes[:, 1] - planes[:, 2]).to(torch.int8).cpu().numpy()
        G, R, C = boards.shape
        s = draw(boards, self.seed)
        moved = torch.from_numpy(transform_boards(boards, s)).to(planes.device)
        policy, value = self.inner(self.pkg.engine.encode_planes(moved))
        maps = np.stack([cell_map(R, C, k) for k in range(group_size(R, C))])
        index = torch.from_numpy(maps[s.astype(np.int64)]).to(planes.device)
        return torch.gather(policy, 1, index).contiguous(), value
