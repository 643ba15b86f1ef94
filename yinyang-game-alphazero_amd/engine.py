"""Torch-tensor level binding of the HIP hot path (include/yy_engine.h).

PyTorch is plumbing here: it owns the HBM tensors and the stream; every operation below is a
hand-written gfx950 kernel in csrc/*.hip.  No CPU fallback exists: tensors must be on a
ROCm device and the extension must be built, otherwise these functions raise.
"""
import ctypes as ct

import numpy as np
import torch

from . import _lib
from .options import SHARED_EVALUATIONS_DEFAULT_SLOTS, SHARED_EVALUATIONS_HIGH_WATER, forced_k, fpu_r, gumbel_m, shared_slots
from ._lib import FLAG_ALIASED, FLAG_EVAL_SYMMETRY, FLAG_FORCED_PLAYOUTS, FLAG_FPU_REDUCTION, FLAG_GUMBEL_INTERIOR, FLAG_GUMBEL_ROOT, FLAG_SOLVER, FLAG_REUSE_PASS_VALUE, FLAG_KEEP_EVALUATIONS, FLAG_REUSE_TRANSPOSITIONS, FLAG_ROWCOL, MctsConfig, check, lib


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _need(t, dtype, shape=None, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.YYError(-1, f"{name}: expected a ROCm device tensor (the hot path has no CPU fallback)")
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.YYError(-1, f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.YYError(-1, f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _flags(rowcol=False, aliased=False):
    return (FLAG_ROWCOL if rowcol else 0) | (FLAG_ALIASED if aliased else 0)


# ------------------------------------------------------------------ stateless rules kernels
def valid_mask(boards, players, rowcol=False):
    """getValidMoves for a batch (yin_yang_game.py:60-78): int8 [G,R,C], int8 [G] -> uint8 [G,A]."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    _need(players, torch.int8, (G,), "players")
    out = torch.empty((G, R * Cc), dtype=torch.uint8, device=boards.device)
    with torch.cuda.device(boards.device):
        check(lib().yy_rules_valid_mask(_p(boards), _p(players), G, R, Cc, _flags(rowcol), _p(out), _stream()))
    return out


def step_(boards, players, actions, rowcol=False):
    """getNextState IN PLACE (yin_yang_game.py:39-58): boards and players are updated; returns the
    uint8 [G] `placed` bits (illegal placements are silently skipped, the player still flips)."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    _need(players, torch.int8, (G,), "players")
    _need(actions, torch.int32, (G,), "actions")
    placed = torch.empty(G, dtype=torch.uint8, device=boards.device)
    with torch.cuda.device(boards.device):
        check(lib().yy_rules_step(_p(boards), _p(players), _p(actions), G, R, Cc, _flags(rowcol), _p(placed), _stream()))
    return placed


def game_ended(boards, players, rowcol=False, with_counts=False):
    """getGameEnded (yin_yang_game.py:80-110): float64 [G] in {0, 1, -1, 0.0001}."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    _need(players, torch.int8, (G,), "players")
    out = torch.empty(G, dtype=torch.float64, device=boards.device)
    counts = torch.empty((G, 2), dtype=torch.int32, device=boards.device) if with_counts else None
    with torch.cuda.device(boards.device):
        check(lib().yy_rules_game_ended(_p(boards), _p(players), G, R, Cc, _flags(rowcol), _p(out), _p(counts), _stream()))
    return (out, counts) if with_counts else out


def _u64(seed):
    return ct.c_uint64(int(seed) & (2 ** 64 - 1))


def symmetry_key(mode, seed):
    """(mode, seed) of symmetry-randomised evaluation as contexts and books compare it: ("off", None), or ("random", seed
    as the device sees it).  ValueError for another mode."""
    if mode not in ("off", "random"):
        raise ValueError(f'evaluation_symmetry={mode!r}: "off" or "random"')
    return ("off", None) if mode == "off" else ("random", int(0 if seed is None else seed) & (2 ** 64 - 1))


def encode_planes(boards, out=None, symmetry_seed=None):
    """board_to_input for a batch (neural_network.py:156-196): float32 [G,5,R,C].  symmetry_seed (not None): every board is
    encoded under the symmetry drawn for it from that seed (evaluation_symmetry below): the evaluator row a
    BatchedMCTS(evaluation_symmetry="random", symmetry_seed=...) writes for the position."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    if out is None:
        out = torch.empty((G, 5, R, Cc), dtype=torch.float32, device=boards.device)
    _need(out, torch.float32, (G, 5, R, Cc), "out")
    with torch.cuda.device(boards.device):
        if symmetry_seed is None:
            check(lib().yy_encode_planes(_p(boards), G, R, Cc, _p(out), _stream()))
        else:
            check(lib().yy_encode_planes_sym(_p(boards), G, R, Cc, _u64(symmetry_seed), _p(out), _stream()))
    return out


def evaluation_symmetry(boards, seed):
    """The board symmetry every position of int8 [G,R,C] is evaluated under with evaluation_symmetry="random" and this
    symmetry seed: int8 [G], a pure function of (seed, position) from the Philox streams (include/yy_engine.h,
    YY_FLAG_EVAL_SYMMETRY).  Square boards, s in 0 .. 7: np.rot90(board, s & 3), then np.fliplr when s & 4; other boards,
    s in 0 .. 3: np.flipud when s & 1, np.fliplr when s & 2."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    out = torch.empty(G, dtype=torch.int8, device=boards.device)
    with torch.cuda.device(boards.device):
        check(lib().yy_eval_symmetry(_p(boards), G, R, Cc, _u64(seed), _p(out), _stream()))
    return out


def pack_boards(boards):
    """int8 [G,R,C] -> (black, white) uint64-as-int64 [NW,G] word-major bitboards."""
    G, R, Cc = boards.shape
    _need(boards, torch.int8, name="boards")
    nw = (R * Cc + 63) // 64
    black = torch.empty((nw, G), dtype=torch.int64, device=boards.device)
    white = torch.empty((nw, G), dtype=torch.int64, device=boards.device)
    with torch.cuda.device(boards.device):
        check(lib().yy_pack_boards(_p(boards), G, R, Cc, _p(black), _p(white), _stream()))
    return black, white


def unpack_boards(black, white, R, Cc):
    nw, G = black.shape
    _need(black, torch.int64, name="black")
    _need(white, torch.int64, (nw, G), "white")
    boards = torch.empty((G, R, Cc), dtype=torch.int8, device=black.device)
    with torch.cuda.device(black.device):
        check(lib().yy_unpack_boards(_p(black), _p(white), G, R, Cc, _p(boards), _stream()))
    return boards


def mask_terminal_bb(black, white, R, Cc, rowcol=False, out=None):
    """Packed rules kernel: both colours' legal masks + game-ended code from BLACK's view
    (0 ongoing, 1, -1, 2 draw) for bitboards [NW,G]."""
    nw, G = black.shape
    _need(black, torch.int64, name="black")
    _need(white, torch.int64, (nw, G), "white")
    if out is None:
        out = (torch.empty_like(black), torch.empty_like(black),
               torch.empty(G, dtype=torch.int8, device=black.device))
    m1, m2, res = out
    with torch.cuda.device(black.device):
        check(lib().yy_rules_mask_terminal_bb(_p(black), _p(white), G, R, Cc, _flags(rowcol), _p(m1), _p(m2), _p(res), _stream()))
    return m1, m2, res


def bias_act_(x, bias, residual=None, relu=True):
    """In-place fused epilogue on a channels-last bf16 activation tensor [N,C,H,W] (NHWC memory):
    x = relu?(x + bias[c] (+ residual)).  One HIP pass (csrc k_bias_act)."""
    if x.dim() != 4 or not x.is_contiguous(memory_format=torch.channels_last) or x.dtype != torch.bfloat16 or not x.is_cuda:
        raise _lib.YYError(-1, "bias_act_: expected a channels-last bf16 device tensor [N,C,H,W]")
    N, Cc, H, W = x.shape
    if bias.dtype != torch.float32 or bias.numel() != Cc or not bias.is_cuda:
        raise _lib.YYError(-1, "bias_act_: bias must be float32 [C] on the device")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype
                                 or not residual.is_contiguous(memory_format=torch.channels_last)):
        raise _lib.YYError(-1, "bias_act_: residual must match x (channels-last bf16)")
    with torch.cuda.device(x.device):
        check(lib().yy_nn_bias_act_bf16(_p(x), _p(bias), _p(residual), N * H * W, Cc, int(bool(relu)), _stream()))
    return x


def tower_forward(planes, weights, bias, n_layers):
    """Stem + residual tower in one LDS-resident MFMA kernel (csrc/yy_tower.hip: k_tower, k_towerq).
    planes f32 [G,5,R,R] (R = 6, 8 or 12) -> bf16 activations as a channels-last tensor [G,128,R,R]."""
    G, _, R, Cc = planes.shape
    _need(planes, torch.float32, (G, 5, R, Cc), "planes")
    n_chunks = 9 + 18 * (n_layers - 1)
    _need(weights, torch.int16, (n_chunks, 8192), "tower weights")
    _need(bias, torch.float32, (n_layers, 128), "tower bias")
    out = torch.empty((G, R, Cc, 128), dtype=torch.bfloat16, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_bf16(_p(planes), _p(weights), _p(bias), _p(out), G, R, Cc, 128, n_layers, _stream()))
    return out.permute(0, 3, 1, 2)      # NCHW view of NHWC memory == channels_last


def tower_forward_f32(planes, weights, bias, n_layers):
    """Stem + residual tower in exact float32 on the f32 MFMA (csrc/yy_tower_f32.hip).
    planes f32 [G,5,8,8] -> f32 activations as a channels-last tensor [G,128,8,8]."""
    G = planes.shape[0]
    _need(planes, torch.float32, (G, 5, 8, 8), "planes")
    _need(weights, torch.float32, (9 + 36 * (n_layers - 1), 4096), "f32 tower weights")
    _need(bias, torch.float32, (n_layers, 128), "tower bias")
    out = torch.empty((G, 8, 8, 128), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_f32(_p(planes), _p(weights), _p(bias), _p(out), G, 8, 8, 128, n_layers, _stream()))
    return out.permute(0, 3, 1, 2)


def tower_heads_forward_h3r(planes, weights, head_w, bias, n_layers, exps, rows=None, n_rows=None, out=None):
    """The 32x32x16 split-f16 tower of round 2 (csrc/yy_tower_h3r.hip; boards 6x6 / 8x8 / 12x12, 128 channels): the A/B partner
    of tower_g.  planes f32 [G,5,R,R] -> f32 [G,2,32*R*R] head features; weights in the wave-major order of
    network.pack_tower_h3r / pack_heads_h3r; rows / n_rows as for tower_g."""
    G, _, R, Cc = planes.shape
    _need(planes, torch.float32, (G, 5, R, Cc), "planes")
    _need(weights, torch.int16, (9 + 36 * (n_layers - 1), 8192), "wave-major split-f16 tower weights")
    _need(head_w, torch.int16, (2, 8192), "wave-major split-f16 head weights")
    _need(bias, torch.float32, (n_layers + 1, 128), "tower+heads bias")
    if rows is not None:
        _need(rows, torch.int32, (G,), "rows")
        _need(n_rows, torch.int32, (1,), "n_rows")
    if out is None:
        out = torch.empty((G, 2, 32 * R * Cc), dtype=torch.float32, device=planes.device)
    _need(out, torch.float32, (G, 2, 32 * R * Cc), "out")
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_f16x3_regs(_p(planes), _p(weights), _p(head_w), _p(bias), None, _p(out), _p(rows), _p(n_rows), G, R, Cc,
                                           128, n_layers, int(exps[0]), int(exps[1]), int(exps[2]), _stream()))
    return out


def tower_forward_h3r(planes, weights, bias, n_layers, exps):
    """Tower activations f32 [G,128,R,R] (channels-last memory) from the register-ring kernel (tests)."""
    G, _, R, Cc = planes.shape
    _need(planes, torch.float32, (G, 5, R, Cc), "planes")
    _need(weights, torch.int16, (9 + 36 * (n_layers - 1), 8192), "wave-major split-f16 tower weights")
    _need(bias, torch.float32, (n_layers, 128), "tower bias")
    out = torch.empty((G, R, Cc, 128), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_f16x3_regs(_p(planes), _p(weights), None, _p(bias), _p(out), None, None, None, G, R, Cc, 128, n_layers,
                                           int(exps[0]), 0, int(exps[2]), _stream()))
    return out.permute(0, 3, 1, 2)


def tower_g_available(channels):
    """Column-block counts the general split-f16 tower kernel is instantiated for at this channel count."""
    buf = (ct.c_int * 8)()
    n = lib().yy_nn_tower_g_forms(int(channels), buf)
    return [int(buf[i]) for i in range(n)]


def tower_g(planes, weights, bias, n_layers, exps, nb, boards, head_w=None, head_bias=None, rows=None, n_rows=None, out=None,
            gate=(-1, 0x7FFFFFFF), column_layout=False, wave_grid=True):
    """General split-f16 tower (csrc/yy_tower_g.hip): planes f32 [G,5,R,C] (R*C <= 144) with the weights of network.pack_tower_g.
    With head_w / head_bias (pack_heads_g): -> f32 [G,2,32*R*C] = (policy features, value features) in the reference's flatten
    order; without: -> the tower activations f32 [G,CH,R,C] (channels-last memory).  nb column blocks of 16 and `boards` boards
    per workgroup (network.tower_g_forms).  rows int32 [G] / n_rows int32 [1] (device): evaluate planes[rows[i]] for i < n_rows
    into dense row i; gate = (lo, hi): the launch only runs when lo < live rows <= hi.  column_layout=True: never the row-aligned
    column blocks the kernel picks by itself where the form admits them (8x8 with two boards per workgroup; same bits), for A/B
    timing.  wave_grid=False: the row-aligned 8-block form at 128 channels on k_tower_g's one-wave-per-32-channels grid instead
    of the 2x2 wave grid (k_tower_g22; same bits), for A/B timing."""
    G, _, R, Cc = planes.shape
    _need(planes, torch.float32, (G, 5, R, Cc), "planes")
    ch = bias.shape[1]
    nw = ch // 32
    _need(weights, torch.int16, (9 + 9 * nw * (n_layers - 1), ch * 64), "split-f16 tower weights (pack_tower_g)")
    _need(bias, torch.float32, (n_layers, ch), "tower bias")
    if rows is not None:
        _need(rows, torch.int32, (G,), "rows")
        _need(n_rows, torch.int32, (1,), "n_rows")
    heads = head_w is not None
    if heads:
        _need(head_w, torch.int16, (4 * nw * 2 * 512,), "split-f16 head weights (pack_heads_g)")
        _need(head_bias, torch.float32, (64,), "head bias")
        if out is None:
            out = torch.empty((G, 2, 32 * R * Cc), dtype=torch.float32, device=planes.device)
        _need(out, torch.float32, (G, 2, 32 * R * Cc), "out")
    else:
        out = torch.empty((G, R, Cc, ch), dtype=torch.float32, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_g(_p(planes), _p(weights), _p(head_w), _p(bias), _p(head_bias), None if heads else _p(out),
                                  _p(out) if heads else None, _p(rows), _p(n_rows), G, R, Cc, ch, n_layers, int(exps[0]), int(exps[1]),
                                  int(exps[2]), int(nb), int(boards), int(gate[0]), int(gate[1]),
                                  1 if column_layout else 0 if wave_grid else 2,
                                  _stream()))
    return out if heads else out.permute(0, 3, 1, 2)


def tower_g_relu_check(start, count, counts):
    """Test hook (csrc/yy_tower_g.hip): over the float32 bit patterns start .. start + count - 1, add to counts[0] (uint32 as
    int32 [2] on the device) the inputs where the 2x2-grid tower's ReLU differs from relu_keep_nan, and lower counts[1] (read as
    uint32) to the smallest such pattern."""
    _need(counts, torch.int32, (2,), "counts")
    with torch.cuda.device(counts.device):
        check(lib().yy_nn_tower_g_relu_check(int(start) & 0xFFFFFFFF, int(count), _p(counts), _stream()))
    return counts


def fc_heads(feats, wpk, bias, jobs, A, H, exps, n_rows=None, logits=None, hidden=None):
    """policy_fc and value_fc1 on the dense feature rows (csrc/yy_fc_heads.hip): feats f32 [G,2,K] -> (logits f32 [G,A], hidden
    f32 [G,H], bias added); weights / bias / jobs from network.pack_fc_heads, exps = (kw, ka).  n_rows int32 [1] (device): rows
    past it are neither read nor written.  A row's results do not depend on G, n_rows or its position in the batch."""
    G, two, K = feats.shape
    _need(feats, torch.float32, (G, 2, K), "feats")
    _need(jobs, torch.int32, (jobs.shape[0], 4), "jobs")
    ksteps = ((K + 127) // 128) * 4
    _need(wpk, torch.int16, (jobs.shape[0] * ksteps * 4096,), "fc head weights (pack_fc_heads)")
    _need(bias, torch.float32, (A + H,), "fc head bias")
    if n_rows is not None:
        _need(n_rows, torch.int32, (1,), "n_rows")
    if logits is None:
        logits = torch.empty((G, A), dtype=torch.float32, device=feats.device)
        hidden = torch.empty((G, H), dtype=torch.float32, device=feats.device)
    _need(logits, torch.float32, (G, A), "logits")
    _need(hidden, torch.float32, (G, H), "hidden")
    with torch.cuda.device(feats.device):
        check(lib().yy_nn_fc_heads_f16x3(_p(feats), _p(wpk), _p(bias), _p(jobs), jobs.shape[0], _p(logits), _p(hidden), _p(n_rows), G, K,
                                         A, H, int(exps[0]), int(exps[1]), _stream()))
    return logits, hidden


def head_finish_f32(logits, hidden, w2, b2, rows=None, n_rows=None, policy=None, value=None):
    """softmax(logits f32 [G,A]) and tanh(relu(hidden f32 [G,H]) @ w2 + b2) in one HIP pass (csrc k_head_finish_f32);
    with rows / n_rows the result of dense row i lands in row rows[i] of (policy, value) for i < n_rows."""
    G, A = logits.shape
    _need(logits, torch.float32, name="logits")
    _need(hidden, torch.float32, (G, hidden.shape[1]), "hidden")
    _need(w2, torch.float32, (hidden.shape[1],), "w2")
    _need(b2, torch.float32, (1,), "b2")
    if rows is not None:
        _need(rows, torch.int32, (G,), "rows")
        _need(n_rows, torch.int32, (1,), "n_rows")
    if policy is None:
        policy = torch.zeros((G, A), dtype=torch.float32, device=logits.device)
        value = torch.zeros(G, dtype=torch.float32, device=logits.device)
    _need(policy, torch.float32, (G, A), "policy")
    _need(value, torch.float32, (G,), "value")
    with torch.cuda.device(logits.device):
        check(lib().yy_nn_head_finish_f32(_p(logits), _p(hidden), G, A, hidden.shape[1], _p(w2), _p(b2), _p(rows), _p(n_rows),
                                          _p(policy), _p(value), _stream()))
    return policy, value


def compact_rows(flags, rows=None, n=None):
    """uint8 [G] flags -> (rows int32 [G], n int32 [1]): rows[:n] = ascending indices of the non-zero flags."""
    G = flags.shape[0]
    _need(flags, torch.uint8, (G,), "flags")
    if rows is None:
        rows = torch.zeros(G, dtype=torch.int32, device=flags.device)
        n = torch.zeros(1, dtype=torch.int32, device=flags.device)
    _need(rows, torch.int32, (G,), "rows")
    _need(n, torch.int32, (1,), "n")
    with torch.cuda.device(flags.device):
        check(lib().yy_compact_rows(_p(flags), G, _p(rows), _p(n), _stream()))
    return rows, n


def tower_heads_forward(planes, weights, bias, n_layers):
    """Tower + fused 1x1 head convolutions: planes f32 [G,5,R,R] (R = 6, 8 or 12) ->
    bf16 [G,2,32*R*R] = (policy features, value features) in the reference's flatten order."""
    G, _, R, Cc = planes.shape
    _need(planes, torch.float32, (G, 5, R, Cc), "planes")
    n_chunks = 9 + 18 * (n_layers - 1) + 1
    _need(weights, torch.int16, (n_chunks, 8192), "tower+heads weights")
    _need(bias, torch.float32, (n_layers + 1, 128), "tower+heads bias")
    out = torch.empty((G, 2, 32 * R * Cc), dtype=torch.bfloat16, device=planes.device)
    with torch.cuda.device(planes.device):
        check(lib().yy_nn_tower_heads_bf16(_p(planes), _p(weights), _p(bias), _p(out), G, R, Cc, 128, n_layers, _stream()))
    return out


def head_finish(h, A, w2, b2):
    """softmax over the first A columns of h (bf16 [G, A+H]) and tanh(relu(h[:, A:]) @ w2 + b2) in one
    HIP pass (csrc k_head_finish) -> (policy f32 [G,A], value f32 [G])."""
    G, W = h.shape
    _need(h, torch.bfloat16, name="h")
    _need(w2, torch.float32, (W - A,), "w2")
    _need(b2, torch.float32, (1,), "b2")
    policy = torch.empty((G, A), dtype=torch.float32, device=h.device)
    value = torch.empty(G, dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        check(lib().yy_nn_head_finish_bf16(_p(h), G, A, W - A, _p(w2), _p(b2), _p(policy), _p(value), _stream()))
    return policy, value


# ------------------------------------------------------------------ episode-loop random draws (csrc/yy_selfplay.hip)
def root_noise(seed, game_id, ply, draw, mask, alpha):
    """Dirichlet(alpha) noise over the legal cells of the games with draw != 0, keyed by (seed, game_id, ply): float64 [G,A].
    alpha must be positive and finite.  A row whose linear total falls below 2^-900 (small alpha: about 28 % of the rows at
    alpha = 1e-3, k = 2; never at alpha >= 0.06) is normalised in log space, so every drawing row with a legal cell sums to 1."""
    G, A = mask.shape
    _need(game_id, torch.int64, (G,), "game_id")
    _need(ply, torch.int32, (G,), "ply")
    _need(draw, torch.uint8, (G,), "draw")
    _need(mask, torch.uint8, (G, A), "mask")
    out = torch.empty((G, A), dtype=torch.float64, device=mask.device)
    with torch.cuda.device(mask.device):
        check(lib().yy_selfplay_root_noise(ct.c_uint64(int(seed) & (2 ** 64 - 1)), _p(game_id), _p(ply), _p(draw), _p(mask), G, A,
                                           float(alpha), _p(out), _stream()))
    return out


def gumbel_rows(seed, game_ids, plies, A, out=None):
    """Gumbel root search: the Gumbel(0, 1) variable of every action at the root of (game_ids[g], plies[g]), keyed by (seed,
    game id, ply, action) (include/yy_engine.h, yy_selfplay_root_gumbel): float32 [G,A], what BatchedMCTS.set_gumbel takes.
    out: a float32 [G,A] tensor to draw into (the context keeps the pointer of the rows it was given)."""
    G = game_ids.shape[0]
    _need(game_ids, torch.int64, (G,), "game_ids")
    _need(plies, torch.int32, (G,), "plies")
    if out is None:
        out = torch.empty((G, int(A)), dtype=torch.float32, device=game_ids.device)
    _need(out, torch.float32, (G, int(A)), "out")
    with torch.cuda.device(game_ids.device):
        check(lib().yy_selfplay_root_gumbel(ct.c_uint64(int(seed) & (2 ** 64 - 1)), _p(game_ids), _p(plies), G, int(A), _p(out),
                                            _stream()))
    return out


def sample_actions(seed, game_id, ply, searching, pi, mask, temperature_threshold):
    """The move choice of play_game (self_play.py:143-160), keyed by (seed, game_id, ply): int32 [G], -1 where not searching."""
    G, A = mask.shape
    _need(game_id, torch.int64, (G,), "game_id")
    _need(ply, torch.int32, (G,), "ply")
    _need(searching, torch.uint8, (G,), "searching")
    _need(pi, torch.float64, (G, A), "pi")
    _need(mask, torch.uint8, (G, A), "mask")
    out = torch.empty(G, dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        check(lib().yy_selfplay_sample_actions(ct.c_uint64(int(seed) & (2 ** 64 - 1)), _p(game_id), _p(ply), _p(searching), _p(pi),
                                               _p(mask), G, A, int(temperature_threshold), _p(out), _stream()))
    return out


def draw_budgets(seed, game_id, ply, searching, p_full, full_sims, fast_sims):
    """Playout-cap draw, keyed by (seed, game_id, ply): one uniform u per searching game, is_full = u < p_full -> (budgets int32
    [G] = full_sims or fast_sims, 0 where not searching; is_full uint8 [G]).  budgets is what BatchedMCTS.run_search takes."""
    G = game_id.shape[0]
    _need(game_id, torch.int64, (G,), "game_id")
    _need(ply, torch.int32, (G,), "ply")
    _need(searching, torch.uint8, (G,), "searching")
    budgets = torch.empty(G, dtype=torch.int32, device=game_id.device)
    is_full = torch.empty(G, dtype=torch.uint8, device=game_id.device)
    with torch.cuda.device(game_id.device):
        check(lib().yy_selfplay_draw_budgets(ct.c_uint64(int(seed) & (2 ** 64 - 1)), _p(game_id), _p(ply), _p(searching), G,
                                             float(p_full), int(full_sims), int(fast_sims), _p(budgets), _p(is_full), _stream()))
    return budgets, is_full


# ------------------------------------------------------------------ free-running self-play (csrc/yy_selfplay_move.hip)
class SelfPlayRun:
    """The device state of a free-running self-play run on one BatchedMCTS context (include/yy_engine.h, yy_selfplay_run_*):
    per-slot games and example histories, the noise array, the counters and the example buffer of `example_capacity` rows.
    arm() starts a run; step(policy, value) is one capturable step (tree step with root noise + the move kernel);
    poll_counters() enqueues an asynchronous copy of the counters into pinned memory; examples(n) copies the first n rows out."""

    COUNTERS = ("started", "finished", "failed", "positions", "recorded", "rows", "overflow", "target")

    def __init__(self, ctx, seed, num_simulations, example_capacity, dirichlet_alpha=0.3, dirichlet_epsilon=0.25,
                 temperature_threshold=10, fast_simulations=None, full_search_probability=1.0):
        self.ctx, self.capacity = ctx, int(example_capacity)
        cfg = _lib.SelfPlayConfig(int(seed) & (2 ** 64 - 1), float(dirichlet_alpha), float(dirichlet_epsilon),
                                  float(full_search_probability), int(temperature_threshold), int(num_simulations),
                                  int(fast_simulations or 0), 0, self.capacity)
        h = ct.c_void_p()
        with torch.cuda.device(ctx.device):
            check(lib().yy_selfplay_run_create(ctx._h, ct.byref(cfg), ct.byref(h)))
        self._h = h
        self.host, self._flip = torch.zeros((2, len(self.COUNTERS)), dtype=torch.int64).pin_memory(), 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.ctx.device)
            lib().yy_selfplay_run_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arm(self, num_games, first_game_index=0, stride=1):
        ctx = self.ctx
        with torch.cuda.device(ctx.device):
            check(lib().yy_selfplay_run_arm(ctx._h, self._h, int(num_games), int(first_game_index), int(stride), _p(ctx.planes),
                                            _p(ctx.needs_eval), _stream()))

    def step(self, policy, value):
        ctx = self.ctx
        _need(policy, torch.float32, (ctx.rows, ctx.A), "policy")
        _need(value, torch.float32, (ctx.rows,), "value")
        with torch.cuda.device(ctx.device):
            check(lib().yy_mcts_step_selfplay(ctx._h, self._h, _p(policy), _p(value), _p(ctx.planes), _p(ctx.needs_eval), _stream()))

    def poll_counters(self):
        """Enqueue the copy of the counters into one of two pinned records (alternating, so that the poll in flight never
        writes the record being read) and return (event recorded behind the copy, record): the record is valid once
        event.query() / event.synchronize() says so.  No device synchronisation."""
        self._flip ^= 1
        host = self.host[self._flip]
        with torch.cuda.device(self.ctx.device):
            check(lib().yy_selfplay_run_counters(self._h, ct.c_void_p(host.data_ptr()), _stream()))
        event = torch.cuda.Event()
        event.record()
        return event, host

    def counters(self, host):
        """A completed poll's record as a dict."""
        return dict(zip(self.COUNTERS, (int(x) for x in host.tolist())))

    def examples(self, n):
        """The first n rows of the example buffer (the order in which games finished) as the engine's example dict."""
        ctx, dev, n = self.ctx, self.ctx.device, int(n)
        out = dict(states=torch.empty((n, ctx.R, ctx.C), dtype=torch.int8, device=dev),
                   policies=torch.empty((n, ctx.A), dtype=torch.float32, device=dev),
                   values=torch.empty(n, dtype=torch.float32, device=dev),
                   game_id=torch.empty(n, dtype=torch.int64, device=dev), ply=torch.empty(n, dtype=torch.int64, device=dev))
        with torch.cuda.device(dev):
            check(lib().yy_selfplay_run_examples(self._h, 0, n, _p(out["states"]), _p(out["policies"]), _p(out["values"]),
                                                 _p(out["game_id"]), _p(out["ply"]), _stream()))
        return out


# ------------------------------------------------------------------ shared book of pre-evaluated opening positions
class OpeningBook:
    """Every position with at most `max_stones` stones that alternating legal play reaches from the empty board (8x8: 770 232
    for max_stones = 8), evaluated ONCE with `evaluator` in batches of `batch` rows and stored as an open-addressing table in
    HBM [position -> policy row f32[A], value].  BatchedMCTS.set_book(book) makes every search look its shallow leaves up
    there before asking the evaluator (include/yy_engine.h: yy_mcts_set_book): all games start from the empty board, so the
    first plies of thousands of games walk the same positions.  The evaluator must be the one the searches use, and a
    deterministic function of the row (BatchedEvaluator.row_independent); the results of a search are then unchanged.
    max_positions bounds the table: enumeration stops before the stone count that would exceed it (max_stones is lowered).
    evaluation_symmetry / symmetry_seed: the rows are those of the contexts that will read the book -- with "random" every
    position is shown to the evaluator under its drawn symmetry and the row stored as returned; the book remembers
    (mode, seed) as `symmetry`, and a context of another (mode, seed) refuses it (BatchedMCTS.set_book)."""

    def __init__(self, R, C, evaluator, max_stones, rowcol=False, batch=4096, device=None, max_positions=8_000_000,
                 evaluation_symmetry="off", symmetry_seed=None):
        self.symmetry = symmetry_key(evaluation_symmetry, symmetry_seed)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.R, self.C, self.A, self.max_stones = int(R), int(C), int(R) * int(C), int(max_stones)
        nw = (self.A + 63) // 64
        boards = torch.zeros((1, R, C), dtype=torch.int8, device=dev)
        player, keys, states = 1, [], []
        for _ in range(self.max_stones):                       # breadth-first over stone counts; a side without a move ends a line
            players = torch.full((boards.shape[0],), player, dtype=torch.int8, device=dev)
            vm = valid_mask(boards, players, rowcol)
            n_children = int(vm.sum())                          # before de-duplication: what the expansion below allocates
            if n_children == 0:
                break
            if n_children > 8 * max_positions:                  # a frontier this wide cannot fit the budget: stop BEFORE expanding it
                self.max_stones = len(keys)
                break
            bi, a = vm.nonzero(as_tuple=True)
            child = boards.reshape(-1, self.A)[bi]
            child[torch.arange(bi.numel(), device=dev), a] = player
            black, white = pack_boards(child.view(-1, R, C))
            key = torch.cat([black.t(), white.t()], dim=1).contiguous()                 # [m, 2*NW]
            uniq, inv = torch.unique(key, dim=0, return_inverse=True)
            first = torch.zeros(uniq.shape[0], dtype=torch.int64, device=dev)
            first[inv] = torch.arange(key.shape[0], device=dev)                         # any representative of each position
            if sum(k.shape[0] for k in keys) + uniq.shape[0] > max_positions:           # keep whole stone counts only
                self.max_stones = len(keys)
                break
            boards = child[first].view(-1, R, C).contiguous()
            keys.append(uniq)
            states.append(boards)
            player = -player
        if not keys:
            raise _lib.YYError(-1, "OpeningBook: nothing to store (max_stones < 1 or max_positions too small)")
        self.keys = torch.cat(keys).contiguous()
        boards = torch.cat(states)
        self.n = int(self.keys.shape[0])
        pol = torch.empty((self.n, self.A), dtype=torch.float32, device=dev)
        val = torch.empty(self.n, dtype=torch.float32, device=dev)
        for lo in range(0, self.n, batch):                                              # the evaluations: n / batch launches
            p, v = evaluator(encode_planes(boards[lo:lo + batch].contiguous(), symmetry_seed=self.symmetry[1]))
            pol[lo:lo + batch], val[lo:lo + batch] = p, v
        self.cap = 64
        while self.cap < 6 * self.n:                   # load <= 1/6: next to no probe run reaches the 8-step window
            self.cap *= 2
        self.meta = torch.zeros(self.cap, dtype=torch.int32, device=dev)
        self.table_keys = torch.zeros((self.cap, 2 * nw), dtype=torch.int64, device=dev)
        slot = torch.empty(self.n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib().yy_book_insert(_p(self.keys), self.n, R, C, _p(self.meta), _p(self.table_keys), self.cap, _p(slot), _stream()))
        ok = slot >= 0
        self.stored = int(ok.sum())
        idx = slot[ok].long()
        self.value = torch.zeros(self.cap, dtype=torch.float32, device=dev)
        self.policy = torch.zeros((self.cap, self.A), dtype=torch.float32, device=dev)
        self.value[idx] = val[ok]
        self.policy[idx] = pol[ok]
        self.bytes = sum(t.numel() * t.element_size() for t in (self.meta, self.table_keys, self.value, self.policy))


# ------------------------------------------------------------------ shared evaluation table: the book the games write themselves
class SharedEvaluations:
    """A shared evaluation table (include/yy_engine.h, yy_mcts_set_shared_evaluations): an open-addressing table in HBM
    [position -> policy row f32[A], value] that the games of ONE BatchedMCTS context fill while they play.  Every fresh
    evaluator row of a non-root leaf is inserted, and a leaf whose position any game of the context had evaluated in an earlier
    launch is served from it without an evaluator row -- the opening book's sharing between games without its build phase,
    stone limit or board-size limit, paid for only in positions that were visited.  Insert-only: no eviction; a full probe
    window drops the insert.  One table per context (never two contexts or two streams on one table), one network and one
    (evaluation_symmetry, symmetry_seed) per table: `symmetry` is compared by BatchedMCTS.set_shared_evaluations, and
    clear() is the caller's job when the network changes.
    slots: rounded up to a power of two; None = SHARED_EVALUATIONS_DEFAULT_SLOTS = 2^23, which at 8x8 costs what the 8-stone
    opening book costs (2.3 GB) -- a starting point, not a measured optimum.
    replace=True (yy_mcts_set_shared_evaluations_replacing): the table that does not fill up.  A slot's claim word (`claim`,
    u64 in the place of `meta`) holds the inserting launch's stamp and a 32-bit tag of the position, so of all games that
    insert one position in one launch exactly one takes a slot (the others count as `duplicates`); a hit leaves the launch's
    stamp in the slot's `last_hit` word; and sweep() -- launches of its own between two tree steps, called by the engines --
    evicts, once more than high_water * slots entries are live, every entry neither inserted nor served since the last sweep
    above that mark.  high_water (a fraction of the slots, an attribute that may be changed between sweeps): None =
    options.SHARED_EVALUATIONS_HIGH_WATER; profiles/shared_evaluations_replace.json holds the comparison it was taken from.
    12 bytes a slot more than the insert-only table.  The same games either way."""

    COUNTERS = ("hits", "inserts", "dropped")
    COUNTERS_EX = COUNTERS + ("duplicates", "evicted", "live")
    TOMBSTONE = 0xFFFFFFFF

    def __init__(self, rows, cols, slots=None, device=None, evaluation_symmetry="off", symmetry_seed=None, replace=False,
                 high_water=None):
        self.symmetry = symmetry_key(evaluation_symmetry, symmetry_seed)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.R, self.C, self.A = int(rows), int(cols), int(rows) * int(cols)
        self.slots = shared_slots(True if slots is None else slots)
        if not self.slots:
            raise ValueError("SharedEvaluations: slots must be positive")
        nw, dev = (self.A + 63) // 64, self.device
        self.replace = bool(replace)
        self.high_water = float(SHARED_EVALUATIONS_HIGH_WATER if high_water is None else high_water)
        if not 0.0 <= self.high_water <= 1.0:
            raise ValueError(f"SharedEvaluations: high_water={high_water} is a fraction of the slots, in [0, 1]")
        if self.replace:
            self.claim = torch.zeros(self.slots, dtype=torch.int64, device=dev)
            self.last_hit = torch.zeros(self.slots, dtype=torch.int32, device=dev)
            self.sweep_state = torch.zeros(8, dtype=torch.int64, device=dev)
            self.meta = None
        else:
            self.meta = torch.zeros(self.slots, dtype=torch.int32, device=dev)
        self.keys = torch.empty((self.slots, 2 * nw), dtype=torch.int64, device=dev)
        self.value = torch.empty(self.slots, dtype=torch.float32, device=dev)
        self.policy = torch.empty((self.slots, self.A), dtype=torch.float32, device=dev)
        self.stamp = torch.ones(1, dtype=torch.int32, device=dev)        # the step stamp: never 0, advanced on the device
        self.ctx = None                                                   # the one context that reads and writes the table

    @property
    def memory_bytes(self):
        own = (self.claim, self.last_hit, self.sweep_state) if self.replace else (self.meta,)
        return sum(t.numel() * t.element_size() for t in own + (self.keys, self.value, self.policy, self.stamp))

    def stamps(self):
        """The insert stamp of every slot (int64 [slots]; 0: never used, TOMBSTONE: evicted)."""
        return (self.claim & 0xFFFFFFFF) if self.replace else (self.meta.to(torch.int64) & 0xFFFFFFFF)

    def live(self):
        """bool [slots]: the slots that hold an entry."""
        st = self.stamps()
        return (st != 0) & (st != self.TOMBSTONE)

    def sweep(self):
        """replace=True only (RuntimeError otherwise): enqueue one sweep on the current stream, which must be the stream of the
        table's context, between two tree steps (never inside a captured step).  No host sync.  Legal with selects pending."""
        if not self.replace:
            raise RuntimeError("SharedEvaluations.sweep(): an insert-only table has no eviction (replace=True)")
        if self.ctx is None:
            return                                                        # no context has ever written to it: nothing to evict
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_shared_evaluations_sweep(self.ctx._h, int(self.high_water * self.slots), _stream()))

    def clear(self):
        """Empty the table (asynchronous, on the current stream: call it on the stream of the table's context).  Through the
        context that holds the table, which refuses while a search is in progress (a pending leaf may name a slot); a
        context armed for a free-running run stays in that state."""
        if self.ctx is None:
            (self.claim if self.replace else self.meta).zero_()
            return
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_shared_evaluations_clear(self.ctx._h, _stream()))

    def fill(self):
        """sync; slots in use."""
        return int(self.live().sum())

    def counters(self):
        """sync; {hits, inserts, dropped} of the table's context since it was made / its last reset_counters(); replace=True:
        also duplicates, evicted and live (the entries the last sweep left)."""
        if self.ctx is None:
            return dict.fromkeys(self.COUNTERS_EX if self.replace else self.COUNTERS, 0)
        return self.ctx.shared_counters_ex() if self.replace else self.ctx.shared_counters()


# ------------------------------------------------------------------ batched MCTS context
class BatchedMCTS:
    """G games searched in lockstep on one GPU; replaces Node + MCTS.search/_simulate
    (ai/mcts.py:28-225, 275-414).  One game per wavefront; see csrc/yy_engine.hip."""

    gumbel_interior = False                # a context's own once created; run_search reads it

    COUNTERS = ("evals", "levels", "children_scanned", "children_created", "terminal_revisits", "nodes", "reused_values",
                "transposition_hits")

    def __init__(self, G, R, C, max_sims, cpuct=1.0, aliased=False, rowcol=False, device=None,
                 edges_per_game=0, nodes_per_game=0, reuse_pass_value=False, reuse_transpositions=False,
                 keep_evaluations=False, leaves_per_step=1, evaluation_symmetry="off", symmetry_seed=None, forced_playouts=None,
                 fpu_reduction=None, fpu_reduction_root=None, solver=False, gumbel_root=None, gumbel_c_visit=None,
                 gumbel_c_scale=None, gumbel_interior=False):
        """gumbel_interior=True (only with gumbel_root, not with fpu_reduction; default off: every launch is what it is without
        the option, the plain Gumbel root search included): v_mix and completed-Q selection below the root
        (YY_FLAG_GUMBEL_INTERIOR, include/yy_engine.h).  The root keeps the evaluator's value of its position -- expand_root()
        then needs value=, which run_search passes --, root_policy() completes unvisited children with v_mix, and a descent
        below the root takes the child of largest pi'(a) - N(a) / (1 + sum N) instead of the PUCT choice.  Fixed at creation.
        gumbel_root=m in 2 .. 64 (copied boards and leaves_per_step == 1 only, not with forced_playouts or solver; None / 0 =
        off: every launch is what it is without the option; the paper: 16) with gumbel_c_visit (None: 50) and gumbel_c_scale
        (None: 1.0): the Gumbel root search (YY_FLAG_GUMBEL_ROOT, include/yy_engine.h).  The root spends the search's budget by
        sequential halving over the m children of largest g + log P, g the Gumbel rows of set_gumbel() (gumbel_rows() draws
        them; needed before the first search), root_policy() is the completed-Q target softmax(log P + sigma(q)) at both
        temperatures, root_gumbel_action() the move; root_counts() stays raw.  The budget is the search's num_sims (or the
        game's own); advance() is refused.  Fixed at creation.
        solver=True (copied boards and leaves_per_step == 1 only; default off: every launch is what it is without the
        option): the MCTS-Solver (YY_FLAG_SOLVER, include/yy_engine.h).  Terminal results are propagated up the tree as proven
        WIN / LOSS / DRAW statuses, a descent that reaches a proven node below the root stops there without an evaluator row,
        and the root keeps being searched; root_proven() and solver_counters() read the proofs.  Fixed at creation.
        fpu_reduction=r > 0 (None / 0 = off: every launch is what it is without the option; KataGo: 0.2), fpu_reduction_root
        (None: r; KataGo: 0 at a noised root): first-play urgency reduction (YY_FLAG_FPU_REDUCTION, include/yy_engine.h).  A child
        that has not been visited is scored with the mean value of its visited siblings less r * sqrt(their share of the prior)
        instead of q = 0; the root uses fpu_reduction_root.  Every board semantics and leaves_per_step.  Fixed at creation.
        forced_playouts=k > 0 (copied boards and leaves_per_step == 1 only; None / 0 = off: every launch is what it is without
        the option; KataGo: 2): forced playouts with policy target pruning at the root (YY_FLAG_FORCED_PLAYOUTS, include/yy_engine.h).
        A visited root child is visited again while N * N < k * P * S, and root_policy() is computed from the pruned counts;
        root_counts() stays raw.  Fixed at creation (captured steps hold the context's device view by value).
        evaluation_symmetry="random" (copied boards only; default "off": every launch is what it is without the option):
        every position is shown to the evaluator under a board symmetry drawn from (symmetry_seed, position) and its policy
        row mapped back (YY_FLAG_EVAL_SYMMETRY, include/yy_engine.h; evaluation_symmetry() above gives the draw).  symmetry_seed
        None = 0.
        reuse_pass_value (copied boards only): a childless non-terminal node keeps the value of its first
        evaluation instead of being evaluated again on every visit (YY_FLAG_REUSE_PASS_VALUE, include/yy_engine.h);
        needs a deterministic evaluator whose row results do not depend on the rest of the batch.
        reuse_transpositions: a leaf whose position was already evaluated in this search takes the cached policy row and
        value instead of an evaluator row (YY_FLAG_REUSE_TRANSPOSITIONS); same requirement.
        keep_evaluations: the cache also serves the later searches of the context (YY_FLAG_KEEP_EVALUATIONS): every search
        must then use the same evaluator -- call clear_evaluation_cache() when the network changes.
        leaves_per_step K > 1: every step runs K descents per game with virtual visits and sends up to G*K leaf rows to the
        evaluator (row g*K + j = descent j of game g; include/yy_engine.h), so a search of num_sims simulations takes
        ceil(num_sims / K) steps.  Copied boards only, no evaluation reuse.  K = 1 is the reference's search."""
        if not torch.cuda.is_available():
            raise _lib.YYError(-100, "BatchedMCTS needs a ROCm device: the hot path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.G, self.R, self.C, self.A = int(G), int(R), int(C), int(R) * int(C)
        self.max_sims, self.cpuct, self.aliased, self.rowcol = int(max_sims), float(cpuct), bool(aliased), bool(rowcol)
        self.reuse_pass_value, self.reuse_transpositions = bool(reuse_pass_value), bool(reuse_transpositions)
        self.keep_evaluations = bool(keep_evaluations)
        self.K = max(1, int(leaves_per_step))
        self.rows = self.G * self.K            # evaluator rows of a step
        self.symmetry = symmetry_key(evaluation_symmetry, symmetry_seed)
        self.forced_playouts = forced_k(forced_playouts)
        self.fpu_reduction, self.fpu_reduction_root = fpu_r(fpu_reduction, fpu_reduction_root)
        self.solver = bool(solver)
        self.gumbel_root, self.gumbel_c_visit, self.gumbel_c_scale = gumbel_m(gumbel_root, gumbel_c_visit, gumbel_c_scale,
                                                                              gumbel_interior)
        self.gumbel_interior = bool(gumbel_interior)
        self._gumbel = None                    # device float32 [G,A] the root expansions read (set_gumbel)
        flags = _flags(rowcol, aliased)
        for flag, on in ((FLAG_REUSE_PASS_VALUE, reuse_pass_value), (FLAG_REUSE_TRANSPOSITIONS, reuse_transpositions),
                         (FLAG_KEEP_EVALUATIONS, keep_evaluations), (FLAG_EVAL_SYMMETRY, self.symmetry[0] == "random"),
                         (FLAG_FORCED_PLAYOUTS, self.forced_playouts), (FLAG_FPU_REDUCTION, self.fpu_reduction),
                         (FLAG_SOLVER, self.solver), (FLAG_GUMBEL_ROOT, self.gumbel_root),
                         (FLAG_GUMBEL_INTERIOR, self.gumbel_interior)):
            flags |= flag if on else 0
        cfg = MctsConfig(self.G, self.R, self.C, self.max_sims, self.cpuct, flags,
                         int(edges_per_game), int(nodes_per_game), int(leaves_per_step), self.symmetry[1] or 0,
                         self.forced_playouts, self.fpu_reduction, self.fpu_reduction_root,
                         self.gumbel_root, self.gumbel_c_visit, self.gumbel_c_scale)
        h = ct.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_create(ct.byref(cfg), ct.byref(h)))
        self._h = h
        self.planes = torch.zeros((self.rows, 5, self.R, self.C), dtype=torch.float32, device=self.device)
        self.needs_eval = torch.zeros(self.rows, dtype=torch.uint8, device=self.device)
        self._num_sims = self.max_sims
        self._budgets = None                   # device int32 [G] the next begin() reads (set_sim_budgets); None: the scalar
        self.book, self.book_version, self._evaluator_owner = None, 0, None
        self.shared = None                     # engine.SharedEvaluations (set_shared_evaluations)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            lib().yy_mcts_destroy(self._h)
            self._h = None
        if getattr(self, "shared", None) is not None:      # table and context name each other: let go, so the arrays are freed now
            self.shared.ctx = None
            self.shared = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory_bytes(self):
        n = ct.c_uint64(0)
        check(lib().yy_mcts_memory_bytes(self._h, ct.byref(n)))
        return n.value

    def steps(self, num_sims):
        """Simulation steps (evaluator calls after the root call) of a search of num_sims simulations."""
        return -(-int(num_sims) // self.K)

    def set_num_sims(self, num_sims):
        """Simulations of the searches begun from now on; K > 1 runs the last step of a search with fewer descents."""
        if int(num_sims) != self._num_sims:
            check(lib().yy_mcts_set_num_sims(self._h, int(num_sims)))
            self._num_sims = int(num_sims)

    def set_sim_budgets(self, budgets):
        """Per-game simulation budgets (device int32 [G], clamped to 0 .. max_sims on the device) of the searches begun from now
        on, or None = every game searches the scalar again.  The context keeps the tensor alive; begin() reads it."""
        if budgets is None and getattr(self, "_budgets", None) is None:
            return
        if budgets is not None:
            _need(budgets, torch.int32, (self.G,), "num_sims")
        check(lib().yy_mcts_set_sim_budgets(self._h, _p(budgets)))
        self._budgets = budgets

    def _sim_budgets(self, num_sims, num_sims_bound):
        """run_search's num_sims -> (the simulation count the host issues steps for, device budgets or None for an int)."""
        if isinstance(num_sims, (int, np.integer)):
            if num_sims > self.max_sims:
                raise _lib.YYError(-1, f"num_sims {num_sims} > max_sims {self.max_sims} the context was sized for")
            return int(num_sims), None
        if isinstance(num_sims, torch.Tensor) and num_sims.device.type != "cpu":
            if num_sims_bound is None:
                raise ValueError("num_sims on the device needs num_sims_bound (an int no budget exceeds): the host counts the steps "
                                 "without reading the tensor")
            if not 0 <= int(num_sims_bound) <= self.max_sims:
                raise ValueError(f"num_sims_bound {num_sims_bound} outside 0 .. max_sims {self.max_sims}")
            return int(num_sims_bound), num_sims
        arr = np.asarray(num_sims.numpy() if isinstance(num_sims, torch.Tensor) else num_sims)
        if arr.shape != (self.G,) or arr.dtype.kind not in "iu":
            raise ValueError(f"num_sims: expected an int or {self.G} integers (one budget per game), got shape {arr.shape} {arr.dtype}")
        if arr.min() < 0 or arr.max() > self.max_sims:
            raise ValueError(f"num_sims: budgets outside 0 .. max_sims {self.max_sims}")
        return int(arr.max()), torch.from_numpy(arr.astype(np.int32)).to(self.device)

    # -- the C ABI, one method per entry point
    def begin(self, boards, root_players, active=None):
        _need(boards, torch.int8, (self.G, self.R, self.C), "boards")
        _need(root_players, torch.int8, (self.G,), "root_players")
        if active is not None:
            _need(active, torch.uint8, (self.G,), "active")
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_begin(self._h, _p(boards), _p(root_players), _p(active), _p(self.planes), _stream()))

    def advance(self, actions):
        """Tree reuse (include/yy_engine.h, yy_mcts_advance): re-root every game's tree at the child of its root under
        actions[g] (device int32 [G]; -1 = keep nothing) after a finished search; may be called again for the opponent's reply.
        Returns kept_visits (device int32 [G]): the visits the new root carries, 0 where the next search starts from a fresh
        root.  The next begin() continues from the kept tree where its board and player are the kept node's, and the search
        tops the root up to its budget.  Copied boards, leaves_per_step == 1."""
        _need(actions, torch.int32, (self.G,), "actions")
        kept = torch.empty(self.G, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_advance(self._h, _p(actions), _p(kept), _stream()))
        self._advanced = True
        return kept

    def expand_root(self, policy, noise=None, eps=0.25, value=None):
        """value: the evaluator's value of the root call, float32 [rows]; a context with gumbel_interior keeps it in the root
        record and needs it, every other context discards it (mcts.py:295)."""
        _need(policy, torch.float32, (self.rows, self.A), "policy")
        if noise is not None:
            _need(noise, torch.float64, (self.G, self.A), "noise")
        with torch.cuda.device(self.device):
            if value is None:
                check(lib().yy_mcts_expand_root(self._h, _p(policy), _p(noise), float(eps), _stream()))
            else:
                _need(value, torch.float32, (self.rows,), "value")
                check(lib().yy_mcts_expand_root_value(self._h, _p(policy), _p(value), _p(noise), float(eps), _stream()))

    def select(self):
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_select(self._h, _p(self.planes), _p(self.needs_eval), _stream()))

    def expand_backup(self, policy, value):
        _need(policy, torch.float32, (self.rows, self.A), "policy")
        _need(value, torch.float32, (self.rows,), "value")
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_expand_backup(self._h, _p(policy), _p(value), _stream()))

    def step(self, policy, value):
        _need(policy, torch.float32, (self.rows, self.A), "policy")
        _need(value, torch.float32, (self.rows,), "value")
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_step(self._h, _p(policy), _p(value), _p(self.planes), _p(self.needs_eval), _stream()))

    def root_counts(self, with_children=False):
        counts = torch.empty((self.G, self.A), dtype=torch.int32, device=self.device)
        cw = torch.empty((self.G, self.A), dtype=torch.float32, device=self.device) if with_children else None
        cp = torch.empty((self.G, self.A), dtype=torch.float32, device=self.device) if with_children else None
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_counts(self._h, _p(counts), _p(cw), _p(cp), _stream()))
        return (counts, cw, cp) if with_children else counts

    def root_policy(self, temperature_zero=False):
        pi = torch.empty((self.G, self.A), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_policy(self._h, int(bool(temperature_zero)), _p(pi), _stream()))
        return pi

    def _read(self, fn, names, *extra):
        """One counter reader of the C ABI, fn(ctx, *extra, out uint64 [len(names)]), as {name: int}."""
        ctr = (ct.c_uint64 * len(names))()
        with torch.cuda.device(self.device):
            check(fn(self._h, *extra, ctr))
        return dict(zip(names, [int(x) for x in ctr]))

    def forced_descents(self):
        """sync; forced_playouts: the root descents, over all games, that took a forced edge since create / reset_counters()."""
        return self._read(lib().yy_mcts_forced_descents, ("forced",))["forced"]

    PROVEN = ("none", "win", "loss", "draw")     # the codes of root_proven(), each for the side to move at that node
    SOLVER_COUNTERS = ("proven_nodes", "proven_descents", "proven_roots")

    def root_proven(self):
        """solver: (root int8 [G], children int8 [G,A]) -- the proven status of every game's root and of the root's children
        by action (0 none, 1 WIN, 2 LOSS, 3 DRAW, each for the side to move at that node: a child that is LOSS is a winning
        move); all 0 without the option.  After a finished search (YYError with a select pending)."""
        root = torch.empty(self.G, dtype=torch.int8, device=self.device)
        child = torch.empty((self.G, self.A), dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_proven(self._h, _p(root), _p(child), _stream()))
        return root, child

    def solver_counters(self):
        """sync; solver: {proven_nodes: nodes proven by propagation, proven_descents: descents that ended on a proven node below
        the root, proven_roots: searches whose root became proven} over all games since create / reset_counters().  After a
        finished search (YYError with a select pending)."""
        return self._read(lib().yy_mcts_solver_counters, self.SOLVER_COUNTERS)

    def set_gumbel(self, rows):
        """Gumbel root search: the Gumbel variables the root expansions read, device float32 [G,A] by action (gumbel_rows()).
        The context keeps the tensor and its pointer: set it before steps are captured and rewrite it in place
        (gumbel_rows(..., out=rows)) before every search."""
        _need(rows, torch.float32, (self.G, self.A), "rows")
        check(lib().yy_mcts_set_gumbel(self._h, _p(rows)))
        self._gumbel = rows

    def root_gumbel(self):
        """Gumbel root search: float32 [G,A], the base score f32(g + log P) of every root child by action; NaN for an action
        without a root edge and for an inactive game."""
        out = torch.empty((self.G, self.A), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_gumbel(self._h, _p(out), _stream()))
        return out

    def root_gumbel_action(self):
        """Gumbel root search: int32 [G], the move -- among the most visited root children the largest g + log P + sigma(q),
        the lowest action on ties; -1 for an inactive game and for a root without children."""
        out = torch.empty(self.G, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_gumbel_action(self._h, _p(out), _stream()))
        return out

    def root_stats(self):
        visits = torch.empty(self.G, dtype=torch.int32, device=self.device)
        wsum = torch.empty(self.G, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_root_stats(self._h, _p(visits), _p(wsum), _stream()))
        return visits, wsum

    def boards(self):
        out = torch.empty((self.G, self.R, self.C), dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_get_boards(self._h, _p(out), _stream()))
        return out

    def tree(self):
        """The trees as they stand (yy_mcts_tree, for tests and tools): (nodes [G,node_cap,4], edges [G,edge_cap,4] -- the 32-bit words
        of the records as int32, named in include/yy_engine.h -- and sizes int32 [G,2] = nodes and edges in use)."""
        caps = (ct.c_int64 * 2)()
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_tree(self._h, None, None, None, caps, None))
        nodes = torch.empty((self.G, caps[0], 4), dtype=torch.int32, device=self.device)
        edges = torch.empty((self.G, caps[1], 4), dtype=torch.int32, device=self.device)
        sizes = torch.empty((self.G, 2), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_tree(self._h, _p(nodes), _p(edges), _p(sizes), caps, _stream()))
        return nodes, edges, sizes

    def status(self):
        """sync; raises YYError(YY_E_ARENA) when a game's arena overflowed; returns the counters."""
        return self._read(lib().yy_mcts_status, self.COUNTERS, None)

    def set_book(self, book):
        """Shallow leaves are looked up in `book` (OpeningBook, or None to unset) before the evaluator is asked; the context
        keeps a reference so that the table outlives its use.  A book built under another (evaluation_symmetry, symmetry_seed)
        holds rows of another frame: ValueError."""
        if book is not None and (book.R, book.C) != (self.R, self.C):
            raise _lib.YYError(-1, "the book was built for another board size")
        if book is not None and getattr(book, "symmetry", ("off", None)) != self.symmetry:
            raise ValueError(f"the book was built with (evaluation_symmetry, symmetry_seed) = {getattr(book, 'symmetry', ('off', None))}, "
                             f"this context evaluates with {self.symmetry}: its rows are in another frame")
        with torch.cuda.device(self.device):
            if book is None:
                check(lib().yy_mcts_set_book(self._h, None, None, None, None, 0, 0))
            else:
                check(lib().yy_mcts_set_book(self._h, _p(book.meta), _p(book.table_keys), _p(book.value), _p(book.policy),
                                             book.cap, book.max_stones))
        self.book = book
        self.book_version += 1      # captured steps hold the table's pointers: LockstepSearch re-captures

    def set_shared_evaluations(self, table):
        """The games of this context share their evaluations through `table` (SharedEvaluations, or None to unset): every fresh
        evaluator row is inserted, and leaves are looked up there after the book and the game's own cache.  Copied boards and
        leaves_per_step == 1 only; with no search in progress, and before steps are captured (captured steps hold the table's
        pointers: LockstepSearch re-captures).  A table belongs to one context; one built for another board or under another
        (evaluation_symmetry, symmetry_seed) is refused (ValueError)."""
        if table is not None:
            if (table.R, table.C) != (self.R, self.C):
                raise ValueError("the shared evaluation table was built for another board size")
            if table.symmetry != self.symmetry:
                raise ValueError(f"the shared evaluation table was built with (evaluation_symmetry, symmetry_seed) = {table.symmetry}, "
                                 f"this context evaluates with {self.symmetry}: its rows are in another frame")
            if table.ctx is not None and table.ctx is not self:
                raise ValueError("the shared evaluation table belongs to another context: one table per context (two contexts on "
                                 "two streams would read each other's unfinished entries)")
            if table.device != self.device:
                raise ValueError("the shared evaluation table lives on another device")
        with torch.cuda.device(self.device):
            if table is None:
                check(lib().yy_mcts_set_shared_evaluations(self._h, None, None, None, None, 0, None))
            elif table.replace:
                check(lib().yy_mcts_set_shared_evaluations_replacing(self._h, _p(table.claim), _p(table.last_hit), _p(table.keys),
                                                                     _p(table.value), _p(table.policy), table.slots,
                                                                     _p(table.stamp), _p(table.sweep_state)))
            else:
                check(lib().yy_mcts_set_shared_evaluations(self._h, _p(table.meta), _p(table.keys), _p(table.value), _p(table.policy),
                                                           table.slots, _p(table.stamp)))
        if self.shared is not None and self.shared is not table:
            self.shared.ctx = None
        if table is not None:
            table.ctx = self
        self.shared = table
        self.book_version += 1      # captured steps hold the table's pointers, like the book's

    def shared_counters(self):
        """sync; shared evaluation table: {hits, inserts, dropped} over all games since create / reset_counters()."""
        return self._read(lib().yy_mcts_shared_counters, SharedEvaluations.COUNTERS)

    def shared_counters_ex(self):
        """sync; shared evaluation table: {hits, inserts, dropped, duplicates, evicted, live}; the last three are 0 for an
        insert-only table."""
        return self._read(lib().yy_mcts_shared_counters_ex, SharedEvaluations.COUNTERS_EX)

    def bind_evaluator(self, evaluator):
        """Evaluations kept across searches (keep_evaluations) and the opening book are results of ONE network: the engine-level
        searches (search.LockstepSearch: SelfPlayEngine, MCTS, Arena) bind the context to their evaluator object; a search with
        another one clears the cache, drops the book and empties the shared evaluation table instead of silently mixing two
        networks' numbers.  The low-level
        search() below takes any callable per call and does not bind: there clear_evaluation_cache() is the caller's job."""
        if self._evaluator_owner is not None and self._evaluator_owner is not evaluator:
            if self.keep_evaluations:
                self.clear_evaluation_cache()
            if self.book is not None:
                self.set_book(None)
            if self.shared is not None:
                self.shared.clear()
        self._evaluator_owner = evaluator

    def clear_evaluation_cache(self):
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_cache_clear(self._h, _stream()))

    def reset_counters(self):
        with torch.cuda.device(self.device):
            check(lib().yy_mcts_reset_counters(self._h, _stream()))

    # -- the whole of MCTS.search for G games (mcts.py:275-343)
    def run_search(self, boards, root_players, num_sims, evaluate, noise=None, eps=0.25, active=None, middle=None,
                   num_sims_bound=None):
        """The ONE statement of a search's C ABI call order; search() below and search.LockstepSearch.run drive it.
        evaluate(root) -> (policy, value) of the leaf batch in self.planes, root=True on the root call (mcts.py:295, value discarded);
        middle(n) issues the n = steps - 1 middle steps (default: n times [evaluate, step]).  num_sims == 0: the root only.
        num_sims: an int (every game; the reference's search), or one budget per game (include/yy_engine.h,
        yy_mcts_set_sim_budgets): a host array-like of G integers in 0 .. max_sims -- the steps of its maximum are issued, a
        game stops selecting once its root holds its budget -- or a device int32 [G] tensor with num_sims_bound, an int no
        budget exceeds (nothing is read back; values are clamped to 0 .. max_sims on the device)."""
        num_sims, budgets = self._sim_budgets(num_sims, num_sims_bound)
        self.set_sim_budgets(budgets)
        if self.K > 1 or getattr(self, "_advanced", False) or getattr(self, "gumbel_root", 0):
            # K > 1: the last step's descents follow from it on the device; K = 1: the budget of a kept root (tree reuse), and
            # the budget that the Gumbel root search plans its halving for
            self.set_num_sims(num_sims)
        self.begin(boards, root_players, active)
        policy, value = evaluate(True)
        # the value of the root call is discarded (mcts.py:295) unless the root keeps it (gumbel_interior: v_mix)
        self.expand_root(policy, noise, eps, **(dict(value=value) if self.gumbel_interior else {}))
        self.select()
        n_steps = self.steps(num_sims)
        if n_steps == 0:
            return
        if middle is not None:
            middle(n_steps - 1)
        else:
            for _ in range(n_steps - 1):
                self.step(*evaluate(False))
        self.expand_backup(*evaluate(False))                   # last simulation: no further select

    def search(self, boards, root_players, evaluator, num_sims, noise=None, eps=0.25, active=None, fused=True,
               num_sims_bound=None):
        """evaluator(planes f32[G*K,5,R,C]) -> (policy f32[G*K,A] softmax, value f32[G*K]) on device.
        Runs 1 + num_sims evaluator calls exactly like the reference (root call, then one per
        simulation; with K leaves per step 1 + ceil(num_sims / K)) and returns the root visit counts int32 [G,A].  fused=False:
        every step but the last as expand_backup + select instead of the fused step kernel.  num_sims / num_sims_bound: run_search's."""
        def unfused(n):
            for _ in range(n):
                self.expand_backup(*evaluator(self.planes))
                self.select()

        self.run_search(boards, root_players, num_sims, lambda root: evaluator(self.planes), noise, eps, active,
                        None if fused else unfused, num_sims_bound)
        return self.root_counts()
