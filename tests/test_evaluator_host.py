"""CPU: the host side of network.py that every evaluator kernel is fed from.  (a) the bits every public packer returns, as
SHA-256 constants recorded at the revision before the packers were given one copy of each shared step; (b) the launches of a
split-f16 evaluator call (which tower forms, with which gates, which buffers) on recording stubs of the engine functions,
after the pattern of tests/test_search_sequence.py; (c) the capability fields of every mode.  Networks are filled from an
integer sequence, not from the random generator, so the bytes do not depend on a torch build.  No GPU."""
import functools
import hashlib

import pytest
import torch

from yinyang_game_alphazero_amd import engine
from yinyang_game_alphazero_amd import network as N
from yinyang_game_alphazero_amd.game import YinYangGame

OPEN = (-1, 0x7FFFFFFF)          # the gate of an ungated tower launch
MODES = ("auto", "f16x3", "f16x3r", "fp32", "fp32t", "bf16", "fp16")


@functools.lru_cache(maxsize=None)
def make_net(R, C, channels, blocks):
    """Every float parameter and buffer = ((arange(n) * 2654435761 + 97 * i) % 2001 - 1000) / 8192 for the i-th tensor of the
    state dict (exact in float32); running_var = |that| + 0.5.  Shared between the tests: never modified."""
    net = N.YinYangNeuralNetwork(YinYangGame(R, C), channels, blocks)
    with torch.no_grad():
        for i, (name, t) in enumerate(net.state_dict().items()):
            if not t.is_floating_point():
                continue
            v = ((torch.arange(t.numel(), dtype=torch.int64) * 2654435761 + 97 * i) % 2001 - 1000).double() / 8192
            if name.endswith("running_var"):
                v = v.abs() + 0.5
            t.copy_(v.reshape(t.shape))
    return net.eval()


def digest(result):
    """SHA-256 over dtype, shape and bytes of every returned tensor and the repr of every returned int."""
    h = hashlib.sha256()
    for x in result:
        if isinstance(x, torch.Tensor):
            h.update(("%s%s" % (x.dtype, tuple(x.shape))).encode())
            h.update(x.contiguous().view(torch.uint8).numpy().tobytes())
        else:
            assert isinstance(x, int), type(x)
            h.update(repr(x).encode())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------ (a) packer bits
ALL = ("pack_tower", "pack_tower_f32", "pack_heads", "pack_tower_h3r", "pack_heads_h3r", "pack_tower_g", "pack_heads_g",
       "pack_fc_heads")
BOARDS = ("pack_tower", "pack_heads", "pack_tower_h3r", "pack_heads_h3r", "pack_tower_g", "pack_heads_g", "pack_fc_heads")
GENERAL = ("pack_tower_g", "pack_heads_g", "pack_fc_heads")
NETS = {"8x8": (8, 8, 128, 2), "6x6": (6, 6, 128, 2), "12x12": (12, 12, 128, 2), "5x7": (5, 7, 32, 1)}
PACKER_CASES = ([("8x8", p) for p in ALL] + [("6x6", p) for p in BOARDS] + [("12x12", p) for p in BOARDS]
                + [("5x7", p) for p in GENERAL])
SHA256 = {
    ('8x8', 'pack_tower'): "80250870bf0607cdda6c3a7d2ab104eb918b219eff7fee0852e00807777819b3",
    ('8x8', 'pack_tower_f32'): "a4c7db96fbe76ec56e7ac17f7c359200728459fa977d98c4938a04007386d58c",
    ('8x8', 'pack_heads'): "265f8440f559a6f35ac2750948026f5f723c118c1fb3bec8ca39dd5ad00e5c52",
    ('8x8', 'pack_tower_h3r'): "b910ab6e3ce0c5a64c30a18f2ac2bc49f24a847964eb2ef8923580d2bc076a18",
    ('8x8', 'pack_heads_h3r'): "a15191e07c825940ea9daab57892f26e005dc81d0e04704a4654ecd39444b6f4",
    ('8x8', 'pack_tower_g'): "ec3b91bf1e676b7b01de84a6e3151c0b417f1f152af9bf69eab823ecd81e0fc5",
    ('8x8', 'pack_heads_g'): "1dbd3122b75a84a08a67b008eedb857f21ec15abfdc4e6686830df6689bf020d",
    ('8x8', 'pack_fc_heads'): "13214f9f9480221b9b251710e4b8e0433ec261e2590e45f87432f227ff9a55dd",
    ('6x6', 'pack_tower'): "80250870bf0607cdda6c3a7d2ab104eb918b219eff7fee0852e00807777819b3",
    ('6x6', 'pack_heads'): "265f8440f559a6f35ac2750948026f5f723c118c1fb3bec8ca39dd5ad00e5c52",
    ('6x6', 'pack_tower_h3r'): "b910ab6e3ce0c5a64c30a18f2ac2bc49f24a847964eb2ef8923580d2bc076a18",
    ('6x6', 'pack_heads_h3r'): "a15191e07c825940ea9daab57892f26e005dc81d0e04704a4654ecd39444b6f4",
    ('6x6', 'pack_tower_g'): "ec3b91bf1e676b7b01de84a6e3151c0b417f1f152af9bf69eab823ecd81e0fc5",
    ('6x6', 'pack_heads_g'): "1dbd3122b75a84a08a67b008eedb857f21ec15abfdc4e6686830df6689bf020d",
    ('6x6', 'pack_fc_heads'): "4ac97867213b9a05122eaea0f3a5ec2860de176626d673c578ee129c5f3b5db9",
    ('12x12', 'pack_tower'): "80250870bf0607cdda6c3a7d2ab104eb918b219eff7fee0852e00807777819b3",
    ('12x12', 'pack_heads'): "265f8440f559a6f35ac2750948026f5f723c118c1fb3bec8ca39dd5ad00e5c52",
    ('12x12', 'pack_tower_h3r'): "b910ab6e3ce0c5a64c30a18f2ac2bc49f24a847964eb2ef8923580d2bc076a18",
    ('12x12', 'pack_heads_h3r'): "a15191e07c825940ea9daab57892f26e005dc81d0e04704a4654ecd39444b6f4",
    ('12x12', 'pack_tower_g'): "ec3b91bf1e676b7b01de84a6e3151c0b417f1f152af9bf69eab823ecd81e0fc5",
    ('12x12', 'pack_heads_g'): "1dbd3122b75a84a08a67b008eedb857f21ec15abfdc4e6686830df6689bf020d",
    ('12x12', 'pack_fc_heads'): "8c118bb1162ef55b183266774157186a3bc6dee511ed1ceef4ca1a0a922a859b",
    ('5x7', 'pack_tower_g'): "79f856aa15e1c01191e4c4e2c29151930c59eef157b030400fb8787bf0c49fb1",
    ('5x7', 'pack_heads_g'): "6fecba8b2f010ef46ff23a229fe53b9be81f43170ff5304629c698d0e13454ca",
    ('5x7', 'pack_fc_heads'): "2071f667c116b067737052c7a48c607ab1f8ed78ba31c654dfc77018ff0b62c7",
    ('8x8', 'fold_batchnorm'): "fbe01cd3afa86883b32db20f046c11247d31fb2cfe4916984b28e19629a03037",
    ('8x8', 'split_f16'): "9fa951d97580311fd1eb85e08deb27b129eb5ae6fc802fbb8add45799061c26a",
    ('8x8', 'evaluator auto'): "e55066f38559b7c579fd7d4f2abc6c9efffcfe83eaeab31dc808fe0c30153a3b",
    ('8x8', 'evaluator f16x3'): "e55066f38559b7c579fd7d4f2abc6c9efffcfe83eaeab31dc808fe0c30153a3b",
    ('8x8', 'evaluator f16x3r'): "27d360cf05c9f7d1167bbc363ac99b870979652144cc7c8dcda58b3c5ed1b26d",
    ('8x8', 'evaluator fp32'): "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
    ('8x8', 'evaluator fp32t'): "efc68e99684228f3157d8cfe83a2f3df6ca3a78f29fe821b831c958fda5e5430",
    ('8x8', 'evaluator bf16'): "c0b45813c3d574085930a70e9e58cca3f6c2050f10bf671f74262f598d5c7565",
    ('8x8', 'evaluator fp16'): "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
}


@pytest.mark.parametrize("net,packer", PACKER_CASES)
def test_packer_returns_the_recorded_bits(net, packer):
    assert digest(getattr(N, packer)(make_net(*NETS[net]))) == SHA256[net, packer]


def test_small_public_helpers():
    """The helpers tests and tools import next to the packers: same values as recorded."""
    net = make_net(*NETS["8x8"])
    assert [c.weight.shape[1] for c, _ in N.tower_convs(net)] == [5, 128, 128, 128, 128]
    assert all(isinstance(bn, torch.nn.BatchNorm2d) for _, bn in N.tower_convs(net))
    assert digest(N.fold_batchnorm(net.conv1, net.bn1)) == SHA256["8x8", "fold_batchnorm"]
    assert digest(N.split_f16(net.policy_fc.weight.detach())) == SHA256["8x8", "split_f16"]
    assert N._pow2_exponent(net.policy_fc.weight.detach()) == 17 and N._pow2_exponent(torch.zeros(3)) == 0
    assert N.ACT_EXP == 3 and N.H3_BOARDS == ((6, 6), (8, 8), (12, 12)) and N.G_MAX_CELLS == 144
    assert N.G_CHANNELS == (32, 64, 96, 128) and (N.G_SPLIT_WG, N.G_HINT_BIG_ONLY, N.G_AUTO_MAX_WG) == (256, 4, 2048)
    assert N.f16x3_covers(net) and N.reference_precision_mode(net) == "f16x3"


# ------------------------------------------------------------------------------------------------------ (b) launch plan
class Stubs:
    """Recording stand-ins for the engine functions a split-f16 evaluator call goes through: each appends to `log` and returns
    the buffers it was given, or fresh tensors where it was given none."""

    NAMES = ("tower_g_available", "tower_g", "tower_heads_forward_h3r", "compact_rows", "fc_heads", "head_finish_f32")

    def __init__(self, monkeypatch):
        self.log = []
        for name in self.NAMES:
            monkeypatch.setattr(engine, name, getattr(self, name))

    def tower_g_available(self, channels):
        return list(range(4, 10)) if channels == 128 else [4, 9]

    def tower_g(self, planes, weights, bias, n_layers, exps, nb, boards, head_w=None, head_bias=None, rows=None, n_rows=None,
                out=None, gate=OPEN):
        self.log.append(("tower_g", (nb, boards), tuple(gate), rows is not None))
        return torch.zeros(1) if out is None else out

    def tower_heads_forward_h3r(self, planes, weights, head_w, bias, n_layers, exps, rows=None, n_rows=None, out=None):
        self.log.append(("tower_heads_forward_h3r", rows is not None))
        return torch.zeros(1) if out is None else out

    def compact_rows(self, flags, rows=None, n=None):
        self.log.append(("compact_rows", rows is not None))
        return (torch.zeros(1), torch.zeros(1)) if rows is None else (rows, n)

    def fc_heads(self, feats, wpk, bias, jobs, A, H, exps, n_rows=None, logits=None, hidden=None):
        self.log.append(("fc_heads", n_rows is not None, logits is not None))
        return (torch.zeros(1), torch.zeros(1)) if logits is None else (logits, hidden)

    def head_finish_f32(self, logits, hidden, w2, b2, rows=None, n_rows=None, policy=None, value=None):
        self.log.append(("head_finish_f32", rows is not None, policy is not None))
        return (torch.zeros(1), torch.zeros(1)) if policy is None else (policy, value)

    def take(self):
        log, self.log = self.log, []
        return log


@pytest.fixture
def stubs(monkeypatch):
    return Stubs(monkeypatch)


def call(ev, G, compacted=False, static=False, R=8):
    planes = torch.zeros((G, 5, R, R))
    return ev(planes, needs_eval=torch.ones(G, dtype=torch.uint8) if compacted else None, static=static)


def dense(form):
    return [("tower_g", form, OPEN, False), ("fc_heads", False, False), ("head_finish_f32", False, False)]


def compacted(*launches):
    return ([("compact_rows", True)] + [("tower_g", form, gate, True) for form, gate in launches]
            + [("fc_heads", True, True), ("head_finish_f32", True, True)])


BIG, SMALL = (8, 2), (4, 1)
PAIR = ((SMALL, (-1, 256)), (BIG, (256, 0x7FFFFFFF)))


def test_forms_and_split_of_the_8x8_evaluator(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    assert (ev.g_big, ev.g_small, ev.g_split) == (BIG, SMALL, 256)


def test_launch_plan_8x8(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    call(ev, 8)
    assert stubs.take() == dense(SMALL)
    call(ev, 256)
    assert stubs.take() == dense(SMALL)
    call(ev, 300)
    assert stubs.take() == dense(BIG)
    for G in (300, 600, 2048):
        call(ev, G, True, "owner")
        assert stubs.take() == compacted(*PAIR), G
    call(ev, 256, True, "owner")
    assert stubs.take() == compacted((SMALL, OPEN))
    call(ev, 2049, True, "owner")
    assert stubs.take() == compacted((BIG, OPEN))
    # compacted without static buffers: fresh row list and results, the same launches
    call(ev, 600, True)
    assert stubs.take() == [("compact_rows", False), ("tower_g", SMALL, (-1, 256), True), ("tower_g", BIG, (256, 0x7FFFFFFF), True),
                            ("fc_heads", True, False), ("head_finish_f32", True, False)]
    # static buffers without compaction: dense launch into the owner's buffers
    call(ev, 300, False, "owner")
    assert stubs.take() == [("tower_g", BIG, OPEN, False), ("fc_heads", False, True), ("head_finish_f32", False, True)]


def test_rows_hint_drops_the_small_form_for_that_owner_only(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    ev.rows_hint("a", 1023.0)
    call(ev, 600, True, "a")
    assert stubs.take() == compacted(*PAIR)
    ev.rows_hint("a", 1024.0)
    call(ev, 600, True, "a")
    assert stubs.take() == compacted((BIG, OPEN))
    call(ev, 600, True, "b")
    assert stubs.take() == compacted(*PAIR)
    call(ev, 200, True, "a")                          # at most g_split rows: the small form whatever the hint
    assert stubs.take() == compacted((SMALL, OPEN))
    ev.rows_hint(True, 1e9)                           # static=True is the shared owner: it has no hint
    call(ev, 600, True, True)
    assert stubs.take() == compacted(*PAIR)


def test_form_key(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    assert ev.form_key("a") == 0
    for rows, key in ((0.0, 0), (511.0, 0), (511.9, 0), (512.0, 1), (4096.0, 1)):
        ev.rows_hint("a", rows)
        assert ev.form_key("a") == key and ev.form_key("unknown") == 0
    fp32 = N.BatchedEvaluator(make_net(*NETS["8x8"]), "fp32")
    fp32.rows_hint("a", 4096.0)
    assert fp32.form_key("a") == 0


def test_thresholds_are_module_constants_read_when_documented(stubs, monkeypatch):
    """G_SPLIT_WG at construction; G_HINT_BIG_ONLY and G_AUTO_MAX_WG at call time."""
    net = make_net(*NETS["8x8"])
    ev = N.BatchedEvaluator(net, "f16x3")
    monkeypatch.setattr(N, "G_SPLIT_WG", 128)
    assert ev.g_split == 256 and N.BatchedEvaluator(net, "f16x3").g_split == 128
    ev.rows_hint("a", 512.0)
    call(ev, 600, True, "a")
    assert stubs.take() == compacted(*PAIR)
    monkeypatch.setattr(N, "G_HINT_BIG_ONLY", 2)
    call(ev, 600, True, "a")
    assert stubs.take() == compacted((BIG, OPEN))
    call(ev, 600, True, "b")
    assert stubs.take() == compacted(*PAIR)
    monkeypatch.setattr(N, "G_AUTO_MAX_WG", 512)
    call(ev, 600, True, "b")
    assert stubs.take() == compacted((BIG, OPEN))


def test_rows_hint_replaced_on_the_class_is_obeyed(stubs, monkeypatch):
    monkeypatch.setattr(N.BatchedEvaluator, "rows_hint", lambda self, owner, mean_rows: None)
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    ev.rows_hint("a", 1e9)
    assert ev.form_key("a") == 0
    call(ev, 600, True, "a")
    assert stubs.take() == compacted(*PAIR)


def test_12x12_has_one_form_and_one_ungated_launch(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["12x12"]), "f16x3")
    assert ev.g_big == ev.g_small == (9, 1) and ev.g_split == 256
    ev.rows_hint("a", 1e9)
    for G in (8, 300):
        call(ev, G, R=12)
        assert stubs.take() == dense((9, 1))
    for G, owner in ((8, "a"), (300, "a"), (300, "b"), (2049, "b")):
        call(ev, G, True, owner, R=12)
        assert stubs.take() == compacted(((9, 1), OPEN)), (G, owner)


def test_5x7_32_channels_forms(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["5x7"]), "auto")
    assert ev.mode == "f16x3" and (ev.g_big, ev.g_small, ev.g_split) == ((9, 4), (4, 1), 256)
    planes = torch.zeros((300, 5, 5, 7))
    ev(planes, needs_eval=torch.ones(300, dtype=torch.uint8), static="a")
    assert stubs.take() == compacted(((4, 1), (-1, 256)), ((9, 4), (256, 0x7FFFFFFF)))


def test_f16x3r_is_mode_f16x3_with_the_h3r_tower(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3r")
    assert ev.mode == "f16x3" and ev.use_h3r
    call(ev, 300)
    assert stubs.take() == [("tower_heads_forward_h3r", False), ("fc_heads", False, False), ("head_finish_f32", False, False)]
    call(ev, 600, True, "a")
    assert stubs.take() == [("compact_rows", True), ("tower_heads_forward_h3r", True), ("fc_heads", True, True),
                            ("head_finish_f32", True, True)]


def test_f16x3r_packs_the_h3_tensors_of_the_public_packers(stubs):
    """The evaluator's h3 attributes against pack_tower_h3r / pack_heads_h3r (themselves pinned above)."""
    net = make_net(*NETS["8x8"])
    ev = N.BatchedEvaluator(net, "f16x3r")
    (wq, bq, kw), (hw, hb, kh) = N.pack_tower_h3r(net), N.pack_heads_h3r(net)
    assert torch.equal(ev.h3r_w, wq) and torch.equal(ev.h3r_hw, hw) and torch.equal(ev.h3_b, torch.cat([bq, hb]))
    assert ev.h3_exps == (kw, kh, N.ACT_EXP) and ev.h3_layers == 5


def test_static_buffers_are_kept_per_batch_height_and_owner(stubs):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), "f16x3")
    a1, a2, b, a3 = call(ev, 300, True, "a"), call(ev, 300, True, "a"), call(ev, 300, True, "b"), call(ev, 600, True, "a")
    assert a1[0] is a2[0] and a1[1] is a2[1]
    assert a1[0] is not b[0] and a1[1] is not b[1] and a1[0] is not a3[0] and a1[1] is not a3[1]
    assert a1[0].shape == (300, 64) and a1[1].shape == (300,) and a3[0].shape == (600, 64)
    t1, t2 = call(ev, 300, True, True), call(ev, 300, False, True)
    assert t1[0] is t2[0] and t1[0] is not a1[0]
    f1, f2 = call(ev, 300, True), call(ev, 300, True)
    assert f1[0] is not f2[0]


@pytest.mark.parametrize("mode", ["fp32", "fp32t", "bf16"])
def test_needs_eval_is_refused_without_compaction(stubs, mode):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), mode)
    with pytest.raises(ValueError, match="^evaluator mode %s does not take needs_eval$" % mode):
        ev(torch.zeros((3, 5, 8, 8)), needs_eval=torch.ones(3, dtype=torch.uint8))


def test_validation_texts_and_order(stubs, monkeypatch):
    with monkeypatch.context() as m:
        for name in ("pack_tower_g", "pack_tower_f32", "pack_fc_heads"):
            m.setattr(N, name, lambda net: pytest.fail("packed before the shape was checked"))
        with pytest.raises(ValueError, match="^f16x3 needs a board of at most 144 cells, 32/64/96/128 channels, at most 10 residual "
                                             "blocks, 32-channel heads$"):
            N.BatchedEvaluator(make_net(5, 29, 32, 1), "f16x3r")
        with pytest.raises(ValueError, match="^fp32t needs 8x8 boards, 128 channels, at most 11 residual blocks$"):
            N.BatchedEvaluator(make_net(*NETS["6x6"]), "fp32t")
    with pytest.raises(ValueError, match="^f16x3r needs 6x6, 8x8 or 12x12 boards and 128 channels$"):
        N.BatchedEvaluator(make_net(*NETS["5x7"]), "f16x3r")
    with pytest.raises(KeyError):
        N.BatchedEvaluator(make_net(*NETS["5x7"]), "int8")


# ------------------------------------------------------------------------------------------------- (c) capability fields
SPLIT = dict(mode="f16x3", tower=False, fused=False, supports_compaction=True, supports_static=True, row_independent=True,
             g_big=BIG, g_small=SMALL, g_split=256, h3_layers=5, n_actions=64, n_hidden=256)
FIELDS = {
    "auto": dict(SPLIT, use_h3r=False),
    "f16x3": dict(SPLIT, use_h3r=False),
    "f16x3r": dict(SPLIT, use_h3r=True),
    "fp32": dict(mode="fp32", tower=False, fused=False),
    "fp32t": dict(mode="fp32t", tower=False, fused=False, f32_layers=5, n_actions=64),
    "bf16": dict(mode="bf16", tower=True, fused=True, fused_heads=True, tower_layers=5, n_actions=64, dtype=torch.bfloat16),
    "fp16": dict(mode="fp16", tower=False, fused=False, dtype=torch.float16),
}
TENSORS = {
    "auto": ("g_w", "g_b", "g_hw", "g_hb", "fc_w", "fc_b", "fc_jobs", "fc2_w", "fc2_b"),
    "f16x3r": ("g_w", "g_b", "g_hw", "g_hb", "fc_w", "fc_b", "fc_jobs", "fc2_w", "fc2_b", "h3_b", "h3r_w", "h3r_hw"),
    "fp32": (),
    "fp32t": ("f32_w", "f32_b", "hconv_w", "hconv_b", "fc_cat_w", "fc_cat_b", "fc2_w", "fc2_b"),
    "bf16": ("tower_w", "tower_b", "towerh_w", "towerh_b", "fc_cat_w", "fc_cat_b", "fc2_w", "fc2_b"),
    "fp16": (),
}
TENSORS["f16x3"] = TENSORS["auto"]
NEUTRAL = dict(supports_compaction=False, supports_static=False, row_independent=False, use_h3r=False, fused_heads=False)


@pytest.mark.parametrize("mode", MODES)
def test_fields_of_each_mode_keep_their_values(stubs, mode):
    net = make_net(*NETS["8x8"])
    ev = N.BatchedEvaluator(net, mode)
    assert ev.net is net and ev.device == torch.device("cpu")
    assert {k: getattr(ev, k) for k in FIELDS[mode]} == FIELDS[mode]
    assert digest([getattr(ev, k) for k in TENSORS[mode]]) == SHA256["8x8", "evaluator " + mode]
    if FIELDS[mode]["mode"] == "f16x3":
        assert ev.g_exps == (N.pack_tower_g(net)[2], N.pack_heads_g(net)[2], N.ACT_EXP)
        assert ev.fc_exps == (N.pack_fc_heads(net)[3], N.ACT_EXP)


def test_bf16_variants(stubs):
    net = make_net(*NETS["8x8"])
    for kw, want in ((dict(tower=False), dict(tower=False, fused=True)),
                     (dict(fused_heads=False), dict(tower=True, fused=True, fused_heads=False)),
                     (dict(fused_epilogue=False), dict(tower=True, fused=False, fused_heads=True))):
        ev = N.BatchedEvaluator(net, "bf16", **kw)
        assert {k: getattr(ev, k) for k in want} == want, kw
    assert not N.BatchedEvaluator(make_net(*NETS["5x7"]), "bf16").tower


@pytest.mark.parametrize("mode", MODES)
def test_every_capability_field_exists_on_every_mode(stubs, mode):
    ev = N.BatchedEvaluator(make_net(*NETS["8x8"]), mode)
    want = dict(NEUTRAL, **{k: v for k, v in FIELDS[mode].items() if k in NEUTRAL})
    assert {k: getattr(ev, k) for k in NEUTRAL} == want
    assert ev._hint == {} and ev._static == {}


def test_fp32_evaluator_runs_the_module(stubs):
    policy, value = N.BatchedEvaluator(make_net(*NETS["8x8"]), "fp32")(torch.zeros((3, 5, 8, 8)))
    assert policy.shape == (3, 64) and value.shape == (3,)
    assert policy.dtype == value.dtype == torch.float32
