"""Golden fixtures stored in parts: no committed file may exceed 1 MiB, so a fixture larger than that is written as
<name>.part0.npz, <name>.part1.npz, ... (compressed), and an array too large for one part is cut along its first axis into
the keys <key>@0, <key>@1, ...  load_parts() returns the arrays exactly as they were given to save_parts()."""
import glob
import os
import re

import numpy as np

PART_BYTES = 768 << 10          # uncompressed bytes per part: stays under 1 MiB even when the data does not compress


def save_parts(base, arrays, part_bytes=PART_BYTES):
    pieces = []
    for k, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= part_bytes or a.ndim == 0:
            pieces.append((k, a))
            continue
        rows = max(1, part_bytes // max(a.nbytes // len(a), 1))
        pieces += [("%s@%d" % (k, i), a[s:s + rows]) for i, s in enumerate(range(0, len(a), rows))]
    parts, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > part_bytes:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    for old in glob.glob(base + ".part*.npz"):
        os.remove(old)
    for i, p in enumerate(parts):
        np.savez_compressed("%s.part%d.npz" % (base, i), **p)


def load_parts(base):
    paths = sorted(glob.glob(base + ".part*.npz"), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    assert paths, base + ".part*.npz: no such fixture"
    flat = {}
    for p in paths:
        with np.load(p) as z:
            flat.update({k: z[k] for k in z.files})
    out, split = {}, {}
    for k, a in flat.items():
        m = re.fullmatch(r"(.*)@(\d+)", k)
        if m:
            split.setdefault(m.group(1), {})[int(m.group(2))] = a
        else:
            out[k] = a
    for k, blocks in split.items():
        out[k] = np.concatenate([blocks[i] for i in range(len(blocks))])
    return out
