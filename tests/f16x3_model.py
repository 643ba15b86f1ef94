"""Float64 models of the split-f16 evaluator ("f16x3": csrc/yy_tower_g.hip, yy_fc_heads.hip, k_head_finish_f32 in
yy_nn_epilogue.hip) and the networks that stress its number format.  Test infrastructure, CPU or device, no GPU kernel.

* `reference_f64`: the module in float64, stage by stage.
* `emulate`: the kernels' arithmetic.  It reads the PACKED operands (network.pack_tower_g / pack_heads_g / pack_fc_heads),
  unpacked from their documented layouts, splits activations with the same hi = f16(x), lo = f16(x - hi) at the same scales
  2^kw / 2^kh / 2^kf / 2^ACT_EXP, forms hi*hi + (lo*hi + hi*lo) exactly in float64 (lo*lo dropped) and rounds to float32
  where the kernels round: the fused epilogue fma, the residual add, the head features, the FC outputs, the float32
  softmax / tanh finish.  It differs from the kernels only by the float32 rounding of their MFMA accumulators.
  `mutant=` selects a deliberately wrong variant (MUTANTS) that the accuracy bounds must reject.
* `make_net(regime, ...)`: seeded networks for the named regimes (REGIMES) and the overflow forms (OVERFLOW_FORMS).
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import oracle_lib as O
from yinyang_game_alphazero_amd import network as N
from yinyang_game_alphazero_amd.game import YinYangGame

ACT_EXP = N.ACT_EXP
F16_LIMIT = 65520.0 / 2 ** ACT_EXP      # an activation at or above this (8190) splits to hi = inf: the format's top
MUTANTS = ("drop_lo_hi", "flush_subnormals", "truncate_split", "bias_act_exp_plus_one")
REGIMES = ("calibrated", "small2", "small3", "large", "wide", "saturated", "flat")
OVERFLOW_FORMS = ("rows", "network", "value_head", "policy_head")


# ---------------------------------------------------------------------------------------------------------- positions
def positions(R, C, G, seed):
    """G positions of random legal play (the CPU oracle), each stopped after a random number of plies: int8 [G,R,C]."""
    rng = np.random.default_rng(seed)
    boards = np.zeros((G, R, C), np.int8)
    players = np.ones(G, np.int8)
    stop = rng.integers(0, R * C + 1, size=G)
    for ply in range(R * C):
        live = stop > ply
        if not live.any():
            break
        m = O.valid_mask(boards, players)
        act = np.array([rng.choice(np.flatnonzero(r)) if r.any() else 0 for r in m], np.int32)
        nb, npl, _ = O.next_state(boards, players, act)
        boards[live], players[live] = nb[live], npl[live]
    return boards


def encode(boards):
    """The evaluator's 5 input planes (CPU oracle): float32 [G,5,R,C]."""
    return torch.from_numpy(O.encode_planes(boards))


# ---------------------------------------------------------------------------------------------------------- split
def _trunc_f16(x):
    """float16 value of x (float64) rounded toward zero (normal and subnormal range; |x| < 65520)."""
    ax = x.abs()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    q = torch.exp2(torch.clamp(e, min=-14.0) - 10.0)                 # f16 quantum at |x|
    return torch.sign(x) * torch.floor(ax / q) * q


def _flush(t):
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def split(x, mutant=None):
    """float32 x -> (hi, lo) as float64 tensors holding float16 values: hi = f16(x), lo = f16(x - hi) (x - hi is exact in f32)."""
    x = x.float()
    if mutant == "truncate_split":
        x64 = x.double()
        hi = _trunc_f16(x64)
        lo = _trunc_f16((x - hi.float()).double())
        return hi, lo
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    hi, lo = hi.double(), lo.double()
    if mutant == "flush_subnormals":
        hi, lo = _flush(hi), _flush(lo)
    return hi, lo


# ---------------------------------------------------------------------------------------------------------- unpacking
def _f16(t):
    return t.contiguous().view(torch.float16).double()


def unpack_tower_g(wq, ch, n_layers):
    """network.pack_tower_g weights -> per layer (hi, lo) float64 [ch, cin_padded, 3, 3].  Chunk [wave ch/32][M block 2][part 2]
    [lane 64][j 8] with cout = wave*32 + mblock*16 + lane%16, cin = kq*32 + (lane//16)*8 + j; chunk order [layer][kq][tap]."""
    nw = ch // 32
    w = _f16(wq).reshape(-1, nw, 2, 2, 4, 16, 8)                      # chunk, wave, mb, part, kg, m, j
    layers, c0 = [], 0
    for li in range(n_layers):
        kq_n = 1 if li == 0 else nw
        t = w[c0:c0 + 9 * kq_n].reshape(kq_n, 9, nw, 2, 2, 4, 16, 8)   # kq, tap, wave, mb, part, kg, m, j
        t = t.permute(4, 2, 3, 6, 0, 5, 7, 1).reshape(2, ch, 32 * kq_n, 3, 3)   # part, cout, cin, ky, kx
        layers.append((t[0], t[1]))
        c0 += 9 * kq_n
    assert c0 == w.shape[0]
    return layers


def unpack_heads_g(hw, ch):
    """network.pack_heads_g -> (hi, lo) float64 [64, ch] (rows 0..31 policy channels, 32..63 value channels).
    Layout [head 2][M block 2][kq ch/32][part 2][lane 64][j 8], channel = mblock*16 + lane%16, cin = kq*32 + (lane//16)*8 + j."""
    nw = ch // 32
    t = _f16(hw).reshape(2, 2, nw, 2, 4, 16, 8)                       # head, mb, kq, part, kg, m, j
    t = t.permute(3, 0, 1, 5, 2, 4, 6).reshape(2, 64, ch)             # part, (head, mb, m), (kq, kg, j)
    return t[0], t[1]


def unpack_fc_heads(fw, jobs, K, A, H):
    """network.pack_fc_heads -> ((hi, lo) float64 [A, K] of policy_fc, (hi, lo) [H, K] of value_fc1, padding).  A job's slice
    is [k-step ceil(K/128)*4][wave 4][part 2][lane 64][j 8], output = first + wave*16 + lane%16, k = kstep*32 + (lane//16)*8 + j.
    `padding` is the largest |value| stored outside the real (output, k) range (must be 0)."""
    ksteps = ((K + 127) // 128) * 4
    w = _f16(fw).reshape(-1, 4096)
    out = [torch.zeros((2, A, K), dtype=torch.float64), torch.zeros((2, H, K), dtype=torch.float64)]
    pad = 0.0
    for head, first, n, blk in jobs.tolist():
        t = w[blk:blk + ksteps].reshape(ksteps, 4, 2, 4, 16, 8)          # kstep, wave, part, kg, m, j
        t = t.permute(2, 1, 4, 0, 3, 5).reshape(2, 64, ksteps * 32)     # part, (wave, m), (kstep, kg, j)
        out[head][:, first:first + n] = t[:, :n, :K]
        pad = max(pad, float(t[:, n:].abs().max()) if n < 64 else 0.0, float(t[:, :, K:].abs().max()) if ksteps * 32 > K else 0.0)
    return (out[0][0], out[0][1]), (out[1][0], out[1][1]), pad


class Packed:
    """Everything the f16x3 evaluator uploads, packed by the product's own functions, plus the unpacked float64 views."""

    def __init__(self, net):
        net = copy.deepcopy(net).cpu().eval()
        self.ch = net.conv1.out_channels
        self.n_layers = 1 + 2 * len(net.res_blocks)
        self.R, self.C = net.board_size
        self.wq, self.bq, self.kw = N.pack_tower_g(net)
        self.hw, self.hb, self.kh = N.pack_heads_g(net)
        self.fw, self.fb, self.jobs, self.kf = N.pack_fc_heads(net)
        self.K = 32 * self.R * self.C
        self.A, self.H = net.policy_fc.out_features, net.value_fc1.out_features
        self.tower = unpack_tower_g(self.wq, self.ch, self.n_layers)
        self.heads = unpack_heads_g(self.hw, self.ch)
        self.fc_p, self.fc_v, self.fc_pad = unpack_fc_heads(self.fw, self.jobs, self.K, self.A, self.H)
        self.fc2_w = net.value_fc2.weight.detach().float().reshape(-1)
        self.fc2_b = net.value_fc2.bias.detach().float().reshape(1)


# ---------------------------------------------------------------------------------------------------------- models
def _relu(t):
    """NaN-preserving ReLU (torch.relu keeps NaN)."""
    return torch.relu(t)


def reference_f64(net, planes):
    """The module in float64 on planes' device: dict of tower [G,CH,R,C], feats [G,2,32*R*C] (policy | value head features),
    logits [G,A], hidden [G,256] (value_fc1 before its ReLU), policy [G,A], value [G]."""
    n64 = copy.deepcopy(net).to(planes.device).double().eval()
    with torch.no_grad():
        x = _relu(n64.bn1(n64.conv1(planes.double())))
        for blk in n64.res_blocks:
            x = blk(x)
        pf = _relu(n64.policy_bn(n64.policy_conv(x))).flatten(1)
        vf = _relu(n64.value_bn(n64.value_conv(x))).flatten(1)
        logits = n64.policy_fc(pf)
        hidden = n64.value_fc1(vf)
        value = torch.tanh(n64.value_fc2(_relu(hidden))).reshape(-1)
        return dict(tower=x, feats=torch.stack([pf, vf], 1), logits=logits, hidden=hidden,
                    policy=torch.softmax(logits, 1), value=value)


def module_f32(net, planes):
    """The float32 module (what mode "fp32" computes) on planes' device, same stages as reference_f64."""
    n32 = copy.deepcopy(net).to(planes.device).float().eval()
    with torch.no_grad():
        x = _relu(n32.bn1(n32.conv1(planes.float())))
        for blk in n32.res_blocks:
            x = blk(x)
        pf = _relu(n32.policy_bn(n32.policy_conv(x))).flatten(1)
        vf = _relu(n32.value_bn(n32.value_conv(x))).flatten(1)
        logits, hidden = n32.policy_fc(pf), n32.value_fc1(vf)
        value = torch.tanh(n32.value_fc2(_relu(hidden))).reshape(-1)
        return dict(tower=x, feats=torch.stack([pf, vf], 1), logits=logits, hidden=hidden,
                    policy=torch.softmax(logits, 1), value=value)


def _mm3(xh, xl, wh, wl, op, mutant):
    """hi*hi + (lo*hi + hi*lo) in float64 (every f16 x f16 product is exact there); lo*lo is dropped as in the kernels."""
    acc1 = op(xh, wh)
    cross = op(xl, wh)
    if mutant != "drop_lo_hi":
        cross = cross + op(xh, wl)
    return acc1 + cross


def emulate(pk, planes, mutant=None):
    """The f16x3 evaluator's arithmetic on planes (float32 [G,5,R,C], any device) -> dict with the stages of reference_f64."""
    dev = planes.device
    d = lambda t: t.to(dev)
    wsplit = (lambda t: _flush(d(t))) if mutant == "flush_subnormals" else d
    G = planes.shape[0]
    s_act = 2.0 ** ACT_EXP
    bias_scale = 2.0 if mutant == "bias_act_exp_plus_one" else 1.0     # bias rows live times 2^ACT_EXP; the mutant uses 2^(ACT_EXP+1)
    x = planes.float() * s_act
    xh, xl = split(x, mutant)
    pad = 32 - xh.shape[1]
    xh, xl = F.pad(xh, (0, 0, 0, 0, 0, pad)), F.pad(xl, (0, 0, 0, 0, 0, pad))
    conv = lambda a, w: F.conv2d(a, w, padding=1)
    res = None
    for L, (wh, wl) in enumerate(pk.tower):
        acc = _mm3(xh, xl, wsplit(wh), wsplit(wl), conv, mutant)
        b = d(pk.bq[L]).double() * bias_scale
        v = (acc * 2.0 ** -pk.kw + b[None, :, None, None]).float()    # fma(acc1 + acc2, 2^-kw, bias): one f32 rounding
        if L > 0 and L % 2 == 0:
            v = v + res                                                # + the f32 skip (f32 add)
        v = _relu(v)
        if L % 2 == 0:
            res = v
        xh, xl = split(v, mutant)
    tower = ((xh + xl).float() * 2.0 ** -ACT_EXP)
    hh, hl = pk.heads
    c1 = lambda a, w: torch.einsum("gchw,oc->gohw", a, w)
    acc = _mm3(xh, xl, wsplit(hh), wsplit(hl), c1, mutant)
    f = _relu((acc * 2.0 ** -(pk.kh + ACT_EXP) + d(pk.hb).double()[None, :, None, None]).float())   # [G, 64, R, C]
    feats = f.reshape(G, 2, -1)
    logits, hidden = emulate_fc(pk, feats, mutant)
    value = torch.tanh(_relu(hidden) @ d(pk.fc2_w) + d(pk.fc2_b))
    return dict(tower=tower, feats=feats, logits=logits, hidden=hidden, policy=torch.softmax(logits, 1), value=value)


def emulate_fc(pk, feats, mutant=None):
    """csrc/yy_fc_heads.hip on feats (float32 [G,2,32*cells]): (logits float32 [G,A], hidden float32 [G,H])."""
    dev = feats.device
    wsplit = (lambda t: _flush(t.to(dev))) if mutant == "flush_subnormals" else (lambda t: t.to(dev))
    out = []
    for head, (wh, wl) in enumerate((pk.fc_p, pk.fc_v)):
        fh, fl = split(feats[:, head].float() * 2.0 ** ACT_EXP, mutant)
        acc = _mm3(fh, fl, wsplit(wh), wsplit(wl), lambda a, w: a @ w.t(), mutant)
        bias = (pk.fb[:pk.A] if head == 0 else pk.fb[pk.A:]).to(dev).double()
        out.append((acc * 2.0 ** -(pk.kf + ACT_EXP) + bias).float())       # fma(acc1 + acc2, 2^-(kf+ka), bias)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------- error measures
STAGES = ("tower", "feats", "logits", "hidden", "policy", "value")


def channel_error(got, ref, stage):
    """Per output channel: max |got - ref| over rows (and cells) divided by max |ref| of that channel.  A channel whose
    reference is exactly zero everywhere must be exactly zero (error 0, else inf).  policy / value: plain max abs error.
    Channels: tower = dim 1; feats = (head, channel) of the [G, 2, 32*cells] layout; logits / hidden = the output column."""
    got, ref = got.double(), ref.double()
    if stage in ("policy", "value"):
        return float((got - ref).abs().max())
    if stage == "tower":
        e, s = (got - ref).abs().transpose(0, 1).flatten(1), ref.abs().transpose(0, 1).flatten(1)
    elif stage == "feats":
        G = got.shape[0]
        e = (got - ref).abs().reshape(G, 64, -1).transpose(0, 1).flatten(1)
        s = ref.abs().reshape(G, 64, -1).transpose(0, 1).flatten(1)
    else:
        e, s = (got - ref).abs().t(), ref.abs().t()
    emax, smax = e.max(1).values, s.max(1).values
    r = torch.where(smax > 0, emax / torch.where(smax > 0, smax, torch.ones_like(smax)),
                    torch.where(emax > 0, torch.full_like(emax, float("inf")), torch.zeros_like(emax)))
    return float(r.max())


def signed_bias(got, ref):
    """sum(got - ref) / sum |ref|: the systematic part of an error (round-to-nearest leaves none; truncation does)."""
    got, ref = got.double(), ref.double()
    return float((got - ref).sum() / ref.abs().sum().clamp_min(1e-300))


def errors(got, ref):
    """Per-stage errors (channel_error) and the signed bias of the tower activations ("tower_bias")."""
    e = {s: channel_error(got[s], ref[s], s) for s in STAGES}
    e["tower_bias"] = abs(signed_bias(got["tower"], ref["tower"]))
    return e


# Error bounds of the f16x3 kernels against float64, per regime and stage (channel_error: per output channel, relative to the
# channel's largest |value|; policy / value absolute; tower_bias: signed_bias of the tower).  The GPU tests apply them to the
# kernels; the emulator must meet them on its own (the format's error) and every MUTANT must break one of them
# (tests/test_f16x3_model.py).  The kernels add float32 accumulation-order error on top of the emulator's.
_B = dict(tower=1e-5, feats=1e-5, logits=2e-5, hidden=2e-5, policy=2e-6, value=1e-5, tower_bias=5e-7)
F64_BOUNDS = {
    "calibrated": dict(_B),
    "small2": dict(_B, tower=2e-4, logits=2e-4, hidden=5e-4),
    "small3": dict(_B, tower=5e-3, logits=2e-4, hidden=1e-3),
    "large": dict(_B),
    "wide": dict(_B),
    "saturated": dict(_B),
    "flat": dict(_B, logits=0.0),
}
# kernel against the emulator: float32 accumulation order only (larger, relative to the channel, where a channel is the small
# difference of large terms: the small regimes' logits / hidden outputs)
_E = dict(tower=1e-5, feats=1e-5, logits=1e-5, hidden=1e-5, policy=3e-6, value=1e-5, tower_bias=1e-7)
EMU_BOUNDS = {r: dict(_E) for r in F64_BOUNDS}
EMU_BOUNDS["small2"].update(tower=1e-4, logits=2e-4, hidden=1e-3)
EMU_BOUNDS["small3"].update(tower=1e-4, logits=2e-4, hidden=1e-3)


# ---------------------------------------------------------------------------------------------------------- networks
def _bns(net, tower_only=False):
    bns = [net.bn1] + [b for blk in net.res_blocks for b in (blk.bn1, blk.bn2)]
    return bns if tower_only else bns + [net.policy_bn, net.value_bn]


def calibrate(net, planes, bns):
    """BatchNorm running statistics of `bns` from ONE train-mode pass over planes (momentum=None: the plain batch statistics)."""
    saved = {}
    for bn in bns:
        saved[bn] = bn.momentum
        bn.momentum = None
        bn.reset_running_stats()
    net.eval()
    for bn in bns:                        # only these normalise by (and record) the batch statistics
        bn.train()
    with torch.no_grad():
        net(planes)
    for bn, m in saved.items():
        bn.momentum = m
    return net.eval()


def max_tower(net, planes, device=None):
    with torch.no_grad():
        planes = planes.to(device) if device is not None else planes
        n64 = copy.deepcopy(net).double().to(planes.device)
        x = torch.relu(n64.bn1(n64.conv1(planes.double())))
        for blk in n64.res_blocks:
            x = blk(x)
    return float(x.max())


def make_net(regime, R, C, ch=128, blocks=10, seed=0, planes=None, form=None, boundary=None, device=None):
    """Seeded YinYangNeuralNetwork (CPU, eval mode) of a named regime (REGIMES, or "overflow" with form in OVERFLOW_FORMS, or
    "boundary" with one tower channel held at the activation `boundary`).  planes: the calibration positions, also the batch
    the "large" regime is sized on (default: 64 positions of random play); device: where that sizing runs its float64 passes."""
    g = torch.Generator().manual_seed(1000 + seed)
    u = lambda shape, a, b: torch.rand(shape, generator=g, dtype=torch.float64).float() * (b - a) + a
    n = lambda shape, s: torch.randn(shape, generator=g, dtype=torch.float64).float() * s
    torch.manual_seed(seed)
    net = N.YinYangNeuralNetwork(YinYangGame(R, C), ch, blocks).eval()
    if planes is None:
        planes = encode(positions(R, C, 64, 7 + seed))
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.copy_(n(m.bias.shape, 0.05))
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(u(m.weight.shape, 0.7, 1.3))
                m.bias.copy_(n(m.bias.shape, 0.1))
        net.policy_fc.bias.copy_(n(net.policy_fc.bias.shape, 0.1))
        net.value_fc1.bias.copy_(n(net.value_fc1.bias.shape, 0.1))
        net.value_fc2.bias.copy_(n(net.value_fc2.bias.shape, 0.1))
        if regime == "wide":
            convs = N.tower_convs(net)
            for conv, bn in convs:
                co = conv.out_channels
                e = u((co,), -14.0, 2.0)
                sign = torch.where(u((co,), 0, 1) < 0.2, -1.0, 1.0)
                bn.weight.copy_(sign * torch.exp2(e))                    # gamma over 2^-14 .. 2^2, some negative
                bn.bias.mul_(torch.exp2(u((co,), -10.0, 0.0)))
                zin = torch.randperm(conv.in_channels, generator=g)[:max(1, conv.in_channels // 16)]
                conv.weight[:, zin] = 0.0                                # input channels whose weights are all zero
        calibrate(net, planes, _bns(net))
        if regime == "wide":
            for conv, bn in N.tower_convs(net):
                co = conv.out_channels
                idx = torch.randperm(co, generator=g)
                dead, zero = idx[:co // 16], idx[co // 16:co // 16 + co // 32]
                # dead channels: running_var = 0, the fold multiplies by 1/sqrt(eps); their weights are small so the outputs are not
                conv.weight[dead] *= float(np.sqrt(bn.eps))
                conv.bias[dead] = bn.running_mean[dead]
                bn.running_var[dead] = 0.0
                # output channels that are exactly zero
                conv.weight[zero] = 0.0
                conv.bias[zero] = 0.0
                bn.running_mean[zero] = 0.0
                bn.bias[zero] = 0.0
        elif regime in ("small2", "small3"):
            s = 1e-2 if regime == "small2" else 1e-3
            for bn in _bns(net, tower_only=True):
                bn.weight.mul_(s)
                bn.bias.mul_(s)
        elif regime == "large":
            # the stem's gamma / beta times f, f found by bisection in log f, until the tower's top lies in [3000, 7000]
            g0, b0 = net.bn1.weight.clone(), net.bn1.bias.clone()
            lo, hi = 0.0, 12.0
            for _ in range(30):
                f = 2.0 ** (0.5 * (lo + hi))
                net.bn1.weight.copy_(g0 * f)
                net.bn1.bias.copy_(b0 * f)
                m = max_tower(net, planes, device)
                if m < 3000.0:
                    lo = np.log2(f)
                elif m > 7000.0:
                    hi = np.log2(f)
                else:
                    break
            calibrate(net, planes, [net.policy_bn, net.value_bn])      # head features back to unit scale
        elif regime == "saturated":
            A = net.policy_fc.out_features
            net.policy_fc.bias.copy_(torch.linspace(-60.0, 60.0, A)[torch.randperm(A, generator=g)])   # logits span > 100
            net.value_fc2.bias.fill_(15.0)                                                              # value pre-activation > 10
        elif regime == "flat":
            net.policy_fc.weight.zero_()                                 # every logit equal
            net.policy_fc.bias.fill_(0.37)
        elif regime == "overflow":
            mid = net.res_blocks[len(net.res_blocks) // 2]
            if form == "network":
                mid.bn2.bias.fill_(1e4)
            elif form == "value_head":
                net.value_bn.bias.fill_(1e4)
            elif form == "policy_head":
                net.policy_bn.bias.fill_(1e4)
            else:
                assert form == "rows", form
        elif regime == "boundary":
            # tower channel 0 holds `boundary` exactly at every cell: stem output constant, no residual-branch contribution, its
            # weights into the next convolutions tiny
            c = 0
            net.conv1.weight[c] = 0.0
            net.conv1.bias[c] = 0.0
            net.bn1.running_mean[c], net.bn1.running_var[c] = 0.0, 1.0 - net.bn1.eps
            net.bn1.weight[c], net.bn1.bias[c] = 1.0, float(boundary)
            for blk in net.res_blocks:
                blk.conv1.weight[:, c] *= 1e-4
                blk.conv2.weight[c] = 0.0
                blk.conv2.bias[c] = 0.0
                blk.bn2.running_mean[c] = 0.0
                blk.bn2.weight[c], blk.bn2.bias[c] = 0.0, 0.0
            net.policy_conv.weight[:, c] *= 1e-4
            net.value_conv.weight[:, c] *= 1e-4
        else:
            assert regime == "calibrated", regime
    return net.eval()


def poison_rows(planes, rows, how):
    """Overflow form (a): the chosen rows' planes times 1e4 ("scale") or NaN ("nan"); returns a new tensor."""
    p = planes.clone()
    for r in rows:
        if how == "nan":
            p[r] = float("nan")
        else:
            p[r] *= 1e4
    return p
