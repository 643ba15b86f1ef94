#!/usr/bin/env python3
"""network.py (packers and BatchedEvaluator) against an earlier copy of the same file: bit comparison of every mode and A/B timing
of the eager evaluator call in ONE process, after the pattern of tools/tower_bf16_ab.py.  Same kernels, same library: tolerance 0.
  python tools/evaluator_ab.py PARENT_NETWORK.py RESULT.json     (PARENT_NETWORK.py: e.g. `git show REV:yinyang-game-alphazero_amd/network.py`
                                                                  saved to a file; loaded as a second module inside the package)"""
import importlib.util, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
# (R, C, channels, modes): every mode on every board it supports
CASES = [(8, 8, 128, ("auto", "f16x3", "f16x3r", "fp32", "fp32t", "bf16", "fp16")),
         (6, 6, 128, ("f16x3", "f16x3r", "fp32", "bf16", "fp16")), (12, 12, 128, ("f16x3", "f16x3r", "fp32", "bf16", "fp16")),
         (5, 7, 32, ("f16x3",))]
HEIGHTS = (5, 300)
ATTRS = ("tower_w", "tower_b", "towerh_w", "towerh_b", "f32_w", "f32_b", "g_w", "g_b", "g_hw", "g_hb", "h3_b", "h3r_w", "h3r_hw",
         "fc_w", "fc_b", "fc_jobs", "fc2_w", "fc2_b", "fc_cat_w", "fc_cat_b", "hconv_w", "hconv_b")
PLAIN = ("mode", "tower", "fused", "tower_layers", "f32_layers", "g_exps", "g_big", "g_small", "g_split", "h3_layers", "h3_exps",
         "fc_exps", "n_actions", "n_hidden")
TIMING = (64, 4096)          # 8x8, f16x3, 128 x 10
MISSING = object()


def main(parent_path, result_path):
    import numpy as np, torch
    import yinyang_game_alphazero_amd as pkg
    from yinyang_game_alphazero_amd import network as child
    spec = importlib.util.spec_from_file_location(pkg.__name__ + ".network_parent", parent_path)
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    E = pkg.engine

    def net_of(R, C, ch, blocks):   # the randomised batch-norm statistics of tests/test_gpu_network.py
        torch.manual_seed(5)
        net = pkg.YinYangNeuralNetwork(pkg.YinYangGame(R, C), ch, blocks).cuda().eval()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0, 0.1); m.running_var.uniform_(0.5, 1.5); m.weight.uniform_(0.7, 1.3); m.bias.normal_(0, 0.1)
                if isinstance(m, torch.nn.Conv2d):
                    m.bias.normal_(0, 0.05)
        return net

    def boards(G, R, C, seed):
        return E.encode_planes(torch.from_numpy(np.random.default_rng(seed).integers(-1, 2, size=(G, R, C)).astype(np.int8)).cuda())

    def same(a, b):
        return bool(torch.equal(a, b) and a.dtype == b.dtype)

    res = dict(box=torch.cuda.get_device_name(0), bits=[], timing=[])
    for R, C, ch, modes in CASES:
        net = net_of(R, C, ch, 2)
        for mode in modes:
            a, b = parent.BatchedEvaluator(net, mode), child.BatchedEvaluator(net, mode)
            rec = dict(board=[R, C], channels=ch, mode=mode)
            rec["attributes"] = [k for k in ATTRS if hasattr(a, k)]
            rec["attributes_equal"] = all(same(getattr(a, k), getattr(b, k)) for k in rec["attributes"])
            rec["plain_equal"] = all(getattr(a, k, MISSING) == getattr(b, k, MISSING) for k in PLAIN if hasattr(a, k))
            for G in HEIGHTS:
                planes = boards(G, R, C, 13 + G)
                # the parent is called twice as well: fp32 / fp16 go through library convolutions and GEMMs, which need not repeat
                # their own bits from call to call; where the parent does not, there is nothing to hold the child to
                (p0, v0), (pa, va), (pb, vb) = [t.clone() for t in a(planes)], a(planes), b(planes)
                rec["dense_%d_parent_repeats" % G] = same(p0, pa) and same(v0, va)
                rec["dense_%d" % G] = same(pa, pb) and same(va, vb) and bool(torch.isfinite(pb).all())
                if getattr(a, "supports_compaction", False):
                    flags = torch.from_numpy((np.random.default_rng(G).random(G) < 0.6).astype(np.uint8)).cuda()
                    (pa, va), (pb, vb) = a(planes, needs_eval=flags, static="owner"), b(planes, needs_eval=flags, static="owner")
                    live = flags.bool()
                    rec["compacted_%d" % G] = same(pa[live], pb[live]) and same(va[live], vb[live]) and bool((pb[live].sum(1) > 0.99).all())
            torch.cuda.synchronize()
            res["bits"].append(rec)
            print(json.dumps(rec), flush=True)
    res["all_bits_equal"] = all(v is True or r.get(k + "_parent_repeats") is False for r in res["bits"] for k, v in r.items()
                                if k not in ("board", "channels", "mode", "attributes") and not k.endswith("_parent_repeats"))
    print("all bits equal:", res["all_bits_equal"], flush=True)
    # timing: eager calls, host and device, stream synchronised around a batch of calls; parent twice per round so that the spread
    # of the parent against itself is measured in the same process; the order rotates from round to round; round 0 is discarded
    net = net_of(8, 8, 128, 10)
    evs = {"parent_a": parent.BatchedEvaluator(net, "f16x3"), "child": child.BatchedEvaluator(net, "f16x3"),
           "parent_b": parent.BatchedEvaluator(net, "f16x3")}
    for G in TIMING:
        planes = boards(G, 8, 8, 2)
        flags = torch.from_numpy((np.random.default_rng(G).random(G) < 0.6).astype(np.uint8)).cuda()
        for kind, kw in (("dense", {}), ("compacted", dict(needs_eval=flags, static="timing"))):
            calls = 200 if G <= 64 else 20
            times = {n: [] for n in evs}
            names = list(evs)
            for r in range(10):
                for n in names[r % 3:] + names[:r % 3]:
                    ev = evs[n]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        ev(planes, **kw)
                    torch.cuda.synchronize()
                    if r:
                        times[n].append((time.perf_counter() - t0) / calls * 1e6)
            med = {n: float(np.median(t)) for n, t in times.items()}
            spread = abs(med["parent_a"] - med["parent_b"])
            med["parent"] = float(np.median(times["parent_a"] + times["parent_b"]))
            rec = dict(G=G, call=kind, calls_per_sample=calls, us_per_call=dict(median=med, min={n: float(np.min(t)) for n, t in times.items()},
                                                                               max={n: float(np.max(t)) for n, t in times.items()}),
                       parent_against_itself_us=spread,
                       child_within_parent_spread_or_lower=med["child"] <= med["parent"] + spread)
            res["timing"].append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(result_path)), exist_ok=True)
    json.dump(res, open(result_path, "w"), indent=1)
    return 0 if res["all_bits_equal"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
