#!/usr/bin/env python3
"""csrc/yy_tower.hip (k_tower and k_towerq in one file) against the revision that had them in two: bit comparison and A/B timing
in ONE process, after the pattern of tools/tg_variants.py.
  python tools/tower_bf16_ab.py build DIR [REV]     (hipcc, no GPU: DIR/libtw_a_parent.so from REV's yy_tower.hip + yy_towerq.hip
                                                     saved with `git show` (default HEAD~1), DIR/libtw_b_child.so from the working tree)
  python tools/tower_bf16_ab.py run DIR RESULT.json (GPU: both libraries through yy_nn_tower_bf16 / yy_nn_tower_heads_bf16)"""
import ctypes as ct, json, os, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "yinyang-game-alphazero_amd"
sys.path.insert(0, ROOT)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"]
# (R, [G ...]): 8x8 reaches k_towerq<8,1>, <8,2> and k_tower; the 6x6 batches have ragged last workgroups and tiles that straddle boards
CASES = [(8, [3, 257, 513]), (6, [5, 19]), (12, [3, 5])]
TIMING = [(8, 4096, "k_tower"), (8, 256, "k_towerq<8,1>"), (8, 512, "k_towerq<8,2>"), (6, 4096, "k_towerq<6,8>"), (12, 4096, "k_towerq<12,2>")]
POISON = 0x7FFF   # a bf16 NaN: no ReLU output


def build(out_dir, rev="HEAD~1"):
    out_dir = os.path.abspath(out_dir)
    par = os.path.join(out_dir, "parent")
    for rel in (PKG + "/csrc/yy_tower.hip", PKG + "/csrc/yy_towerq.hip", PKG + "/csrc/yy_common.h", "include/yy_engine.h"):
        os.makedirs(os.path.dirname(os.path.join(par, rel)), exist_ok=True)
        open(os.path.join(par, rel), "wb").write(subprocess.check_output(["git", "show", "%s:%s" % (rev, rel)], cwd=ROOT))
    stub = os.path.join(out_dir, "stub.cpp")
    open(stub, "w").write('#include <stdio.h>\nextern "C" int yy_tower_set_err(int c, const char *m) { fprintf(stderr, "tower error %d: %s\\n", c, m); return c; }\n')
    srcs = {"a_parent": [os.path.join(par, PKG, "csrc", f) for f in ("yy_tower.hip", "yy_towerq.hip")],
            "b_child": [os.path.join(ROOT, PKG, "csrc", "yy_tower.hip")]}
    procs = [(n, subprocess.Popen(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", os.path.join(out_dir, "libtw_%s.so" % n)] + s + [stub])) for n, s in srcs.items()]
    for n, p in procs:
        assert p.wait() == 0, n
        print("built", n)
    json.dump(dict(parent=subprocess.check_output(["git", "rev-parse", rev], cwd=ROOT).decode().strip(),
                   child_parent=subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()),
              open(os.path.join(out_dir, "revs.json"), "w"))


def run(lib_dir, result_path):
    import numpy as np, torch
    import yinyang_game_alphazero_amd as pkg
    E = pkg.engine
    vp = ct.c_void_p
    libs = {}
    for n in ("a_parent", "b_child"):
        L = ct.CDLL(os.path.join(os.path.abspath(lib_dir), "libtw_%s.so" % n))
        for f in (L.yy_nn_tower_bf16, L.yy_nn_tower_heads_bf16):
            f.argtypes = [vp] * 4 + [ct.c_int] * 5 + [vp]
        libs[n] = L

    def call(L, ev, planes, heads, out=None):
        G, _, R, C = planes.shape
        if out is None:
            out = torch.full((G, 2, 32 * R * C) if heads else (G, R, C, 128), POISON, dtype=torch.int16, device="cuda")
        w, b = (ev.towerh_w, ev.towerh_b) if heads else (ev.tower_w, ev.tower_b)
        fn = L.yy_nn_tower_heads_bf16 if heads else L.yy_nn_tower_bf16
        rc = fn(vp(planes.data_ptr()), vp(w.data_ptr()), vp(b.data_ptr()), vp(out.data_ptr()), G, R, C, 128, ev.tower_layers,
                vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        return out

    def net_of(R, blocks):   # the randomised batch-norm statistics of tests/test_gpu_network.py
        torch.manual_seed(5)
        net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(R, R), 128, blocks).cuda().eval()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.1)
                if isinstance(m, torch.nn.Conv2d):
                    m.bias.normal_(0, 0.05)
        return pkg.BatchedEvaluator(net, "bf16")

    def boards(G, R, seed):
        return E.encode_planes(torch.from_numpy(np.random.default_rng(seed).integers(-1, 2, size=(G, R, R)).astype(np.int8)).cuda())

    res = dict(box=torch.cuda.get_device_name(0), bits=[], timing=[])
    if os.path.exists(os.path.join(lib_dir, "revs.json")):
        res["revisions"] = json.load(open(os.path.join(lib_dir, "revs.json")))
    evs = {}
    for R, Gs in CASES:
        for blocks in (1, 10):
            ev = evs[(R, blocks)] = net_of(R, blocks)
            for G in Gs:
                planes = boards(G, R, 13 + G)
                for heads in (True, False):
                    a, b = call(libs["a_parent"], ev, planes, heads), call(libs["b_child"], ev, planes, heads)
                    torch.cuda.synchronize()
                    rec = dict(board=R, G=G, blocks=blocks, output="out_heads" if heads else "out", same_bits=bool(torch.equal(a, b)),
                               written=bool((a != POISON).all() and (b != POISON).all()), nonzero=bool((b != 0).any()))
                    res["bits"].append(rec)
                    print(json.dumps(rec), flush=True)
    res["all_bits_equal"] = all(r["same_bits"] and r["written"] and r["nonzero"] for r in res["bits"])
    print("all bits equal:", res["all_bits_equal"], flush=True)
    # timing: fused heads, 128 x 10, interleaved rounds in this one process; round 0 is discarded
    for R, G, kernel in TIMING:
        ev, planes = evs[(R, 10)], boards(G, R, 2)
        out = torch.empty((G, 2, 32 * R * R), dtype=torch.int16, device="cuda")
        times = {n: [] for n in libs}
        for r in range(7):
            for n, L in libs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(5):
                    call(L, ev, planes, True, out)
                t1.record(); torch.cuda.synchronize()
                if r:
                    times[n].append(t0.elapsed_time(t1) / 5)
        ms = {n: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for n, t in times.items()}
        rec = dict(kernel=kernel, board=R, G=G, ms=ms, child_within_parent_spread_or_lower=ms["b_child"]["median"] <= ms["a_parent"]["max"])
        res["timing"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(result_path)), exist_ok=True)
    json.dump(res, open(result_path, "w"), indent=1)


if __name__ == "__main__":
    build(*sys.argv[2:4]) if sys.argv[1] == "build" else run(sys.argv[2], sys.argv[3])
