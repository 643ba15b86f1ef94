#!/usr/bin/env python3
"""Build / run variants of csrc/yy_tower_g.hip side by side: bit comparison and A/B timing in ONE process.
  python tools/tg_variants.py build DIR [name=source.hip ...]   (hipcc, no GPU: one libtg_<name>.so per variant in DIR)
  python tools/tg_variants.py run DIR RESULT.json               (GPU: every libtg_*.so in DIR; the first name in sorted order
                                                                 is the yardstick the others are compared with)
A variant is a source file plus extra hipcc flags: an experiment macro placed in csrc/yy_tower_g.hip, or another revision of the
file (e.g. `git show HEAD~1:yinyang-game-alphazero_amd/csrc/yy_tower_g.hip` saved outside git and named on the command line)."""
import ctypes as ct, glob, json, os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "yinyang-game-alphazero_amd", "csrc")
sys.path.insert(0, ROOT)
# name -> source file and extra hipcc flags (the round-3 experiments -- full fragment window, lo-before-hi reads, unrolled channel
# groups, ring depth 3, epilogue fused into a block-major last group, one dual-form launch -- were macros built this way, measured
# against "base" in one process and removed again: DESIGN.md section 3)
VARIANTS = {"base": dict(src=os.path.join(CSRC, "yy_tower_g.hip"), flags=[])}
# bit comparison: (R, C, channels, residual blocks, [(nb, boards, layout)]); G = 37 rows, dense and gathered, heads and activations
CASES = [(8, 8, 128, 10, [(8, 2, 0), (8, 2, 1), (8, 2, 2), (4, 1, 0), (5, 1, 0), (6, 1, 0)]),
         (6, 6, 128, 2, [(9, 4, 0)]), (12, 12, 128, 2, [(9, 1, 0)]), (10, 10, 128, 2, [(7, 1, 0)]), (5, 7, 128, 2, [(9, 4, 0)]),
         (4, 4, 128, 2, [(4, 4, 0)]), (6, 6, 32, 2, [(9, 4, 0), (4, 1, 0)]), (6, 6, 64, 2, [(9, 4, 0), (4, 1, 0)]),
         (6, 6, 96, 2, [(9, 4, 0), (4, 1, 0)])]


def build(out_dir, extra):
    os.makedirs(out_dir, exist_ok=True)
    variants = dict(VARIANTS)
    for e in extra:
        name, src = e.split("=", 1)
        variants[name] = dict(src=os.path.abspath(src), flags=[])
    stub = os.path.join(out_dir, "stub.cpp")
    open(stub, "w").write('#include <stdio.h>\nextern "C" int yy_tower_set_err(int c, const char *m) { fprintf(stderr, "tower error %d: %s\\n", c, m); return c; }\n')
    procs = []
    for name, v in variants.items():
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
               "-I", CSRC, "-o", os.path.join(out_dir, "libtg_%s.so" % name), v["src"], stub] + v["flags"]
        procs.append((name, subprocess.Popen(cmd)))
    for name, p in procs:
        assert p.wait() == 0, name
        print("built", name)


def run(lib_dir, result_path):
    import numpy as np, torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    vp = ct.c_void_p
    libs = {}
    for so in sorted(glob.glob(os.path.join(lib_dir, "libtg_*.so"))):
        L = ct.CDLL(so)
        L.yy_nn_tower_g.argtypes = [vp] * 9 + [ct.c_int] * 13 + [vp]
        libs[os.path.basename(so)[6:-3]] = L
    names = list(libs)
    print("variants:", names, flush=True)

    def call(L, ev, planes, form, heads, rows=None, n=None):
        G, _, R, C = planes.shape
        ch = ev.g_b.shape[1]
        out = torch.full((G, 2, 32 * R * C) if heads else (G, R, C, ch), -7.0, dtype=torch.float32, device="cuda")
        p = lambda t: None if t is None else vp(t.data_ptr())
        hw, hb = (ev.g_hw, ev.g_hb) if heads else (None, None)
        rc = L.yy_nn_tower_g(p(planes), p(ev.g_w), p(hw), p(ev.g_b), p(hb), None if heads else p(out), p(out) if heads else None, p(rows), p(n),
                             G, R, C, ch, ev.h3_layers, int(ev.g_exps[0]), int(ev.g_exps[1]), int(ev.g_exps[2]), form[0], form[1], -1, 0x7FFFFFFF,
                             form[2], vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rc, form)
        return out

    def net_of(R, C, ch, blocks, seed):   # the randomised batch-norm statistics of tests/test_gpu_tower_grid.py::_net
        torch.manual_seed(seed)
        net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(R, C), ch, blocks).cuda().eval()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.1)
                if isinstance(m, torch.nn.Conv2d):
                    m.bias.normal_(0, 0.05)
        return pkg.BatchedEvaluator(net, "f16x3")

    def boards(G, R, C, seed):
        return E.encode_planes(torch.from_numpy(np.random.default_rng(seed).integers(-1, 2, size=(G, R, C)).astype(np.int8)).cuda())

    def same(a, b):   # NaN in the same entries, every other entry bit for bit
        nan = torch.isnan(a)
        return bool(torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan].view(torch.int32), b[~nan].view(torch.int32)))

    res = dict(variants=names, yardstick=names[0], bits=[], timing=[])
    evs = {}
    for R, C, ch, blocks, forms in CASES:
        ev = evs[(R, C, ch)] = net_of(R, C, ch, blocks, 5)
        planes = boards(37, R, C, 13)
        rows, n = E.compact_rows(torch.from_numpy((np.random.default_rng(3).random(37) < 0.5).astype(np.uint8)).cuda())
        k = int(n)
        for form in forms:
            for heads in (True, False):
                for gathered in (False, True):
                    outs = [call(libs[v], ev, planes, form, heads, *((rows, n) if gathered else ())) for v in names]
                    torch.cuda.synchronize()
                    live = k if gathered else 37
                    rec = dict(board=[R, C], channels=ch, blocks=blocks, nb=form[0], boards=form[1], layout=form[2], output="out_heads" if heads else "out",
                               rows="gathered %d of 37" % k if gathered else "dense 37", finite=bool(torch.isfinite(outs[0][:live]).all()),
                               written=bool((outs[0][:live] != -7.0).any(dim=tuple(range(1, outs[0].dim()))).all()),
                               same_bits={v: same(outs[0], o) for v, o in zip(names[1:], outs[1:])})
                    res["bits"].append(rec)
                    print(json.dumps(rec), flush=True)
    # timing: interleaved rounds in this one process; round 0 is discarded
    G = 4096
    ev8 = evs[(8, 8, 128)]
    flags = np.zeros(G, dtype=np.uint8)
    flags[np.random.default_rng(7).choice(G, 1883, replace=False)] = 1
    rows8, n8 = E.compact_rows(torch.from_numpy(flags).cuda())
    jobs = [("8x8 128x10 (8,2) grid dense 4096", ev8, boards(G, 8, 8, 1), (8, 2, 0), None, None),
            ("8x8 128x10 (8,2) grid gathered 1883 of 4096", ev8, boards(G, 8, 8, 1), (8, 2, 0), rows8, n8)]
    for R, C, ch, blocks, forms in CASES:
        for form in forms:
            if (R, C, ch) + form != (8, 8, 128, 8, 2, 0):
                jobs.append(("%dx%d %dx%d (%d,%d) layout %d dense 4096" % ((R, C, ch, blocks) + form), evs[(R, C, ch)], boards(G, R, C, 2), form, None, None))
    for label, ev, planes, form, rows, n in jobs:
        times = {v: [] for v in names}
        for r in range(7):
            for v in names:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(5):
                    call(libs[v], ev, planes, form, True, rows, n)
                t1.record(); torch.cuda.synchronize()
                if r:
                    times[v].append(t0.elapsed_time(t1) / 5)
        rec = dict(case=label, ms={v: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for v, t in times.items()})
        res["timing"].append(rec)
        print(json.dumps(rec), flush=True)
    res["all_bits_equal"] = all(all(r["same_bits"].values()) for r in res["bits"])
    print("all bits equal:", res["all_bits_equal"])
    os.makedirs(os.path.dirname(os.path.abspath(result_path)), exist_ok=True)
    json.dump(res, open(result_path, "w"), indent=1)


if __name__ == "__main__":
    build(sys.argv[2], sys.argv[3:]) if sys.argv[1] == "build" else run(sys.argv[2], sys.argv[3])
