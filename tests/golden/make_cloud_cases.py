#!/usr/bin/env python3
"""Generate tests/golden/g19_cloud_cases.npz from the REFERENCE ITSELF (build container only, needs oracle/_ref).

Run from the repo root:   python tests/golden/make_cloud_cases.py

For every case of tests/cloud_cases.py that the compiled reference core (oracle/_ref/libref.so: the reference's C++
sources compiled unmodified, oracle/Makefile) can run, what it returns:

  sub/<name>/...   subsampling cases with reference=True: the inputs and out_points / out_lens / out_features /
                   out_labels; cases of more than 8 000 points keep out_lens and, under <key>.sha256, the digests of
                   the inputs and of the other outputs (a drift of the NumPy generator then shows as an input mismatch,
                   not as a kernel bug)
  nb/<name>/...    neighbour cases: the inputs, ref_rows, and `out` = the rows on which the reference is a referee
                   (cloud_cases.NbCase) without all-padding columns; matrices of more than 64 KiB as the digest of
                   their tie-canonical form (indices ascending inside groups of equal float32 d2 -- the order the C
                   oracle and the kernels produce), since the reference's own order inside such a group is that of its
                   KD-tree traversal

The reference is never given an empty cloud or ldim = 2 in a batch of several clouds (SIGFPE / std::length_error).
Only DATA is written; no reference source text."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "g19_cloud_cases.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cloud_cases as cc  # noqa: E402
from oracle import cport  # noqa: E402
from util import canon_ties, nb_d2  # noqa: E402


def main():
    assert cport.ref() is not None, "build oracle/_ref first (make -C oracle ref)"
    rec = {}
    for name, c in cc.sub_cases().items():
        if not c.reference:
            continue
        assert (c.lens > 0).all() and (c.labels is None or c.labels.shape[1] < 2 or len(c.lens) == 1), name
        small = len(c.points) <= cc.STORE_POINTS
        for k, a in cc.sub_inputs(c).items():
            cc.put(rec, "sub/%s/%s" % (name, k), a, small or np.ndim(a) == 0 or k == "lens")
        res = cport.subsample_batch(c.points, c.lens, c.features, c.labels, c.dl, c.max_p, impl="ref")
        for k, a in cc.sub_outputs(res, c).items():
            cc.put(rec, "sub/%s/%s" % (name, k), a, small or k == "out_lens")
    for name, c in cc.nb_cases().items():
        for k, a in cc.nb_inputs(c).items():
            cc.put(rec, "nb/%s/%s" % (name, k), a, True)
        rec["nb/%s/ref_rows" % name] = np.int32(c.ref_rows)
        if c.ref_rows == 0:
            continue
        ns = len(c.supports)
        out = cport.radius_neighbors_batch(c.queries, c.supports, c.q_lens, c.s_lens, c.radius, impl="ref")
        out = cc.trim_rows(out, c.ref_rows, ns)
        if out.nbytes <= cc.STORE_BYTES:
            rec["nb/%s/out" % name] = out
        else:
            q = c.queries[:c.ref_rows]
            canon = canon_ties(out, nb_d2(q, c.supports, c.q_lens, c.s_lens, out))
            cc.put(rec, "nb/%s/out_canonical" % name, canon, False)
    np.savez_compressed(OUT, **rec)
    print("wrote %s: %d entries, %d bytes" % (OUT, len(rec), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
