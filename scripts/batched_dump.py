"""Seeded dump of the batched GSM and BaM kernels' outputs, for before / after comparisons of a library change (DESIGN.md
section 9): at eight (D, B) shapes, K = 13 (a tail slot in the four-problem workgroups), the one-shot update, a 20-iteration
fit and a fit with one NaN target, for both methods -- 48 arrays of results.

  python scripts/batched_dump.py OUT.npz                 dump with the library the package loads
  GSMVI_HIP_LIB_VARIANT=old python scripts/batched_dump.py OUT.npz   ... with gsm-vi_amd/libgsmvi_hip_old.so
  python scripts/batched_dump.py --compare A.npz B.npz   bit-for-bit comparison (NaNs compare equal)
"""
import os
import sys

import numpy as np

SHAPES = ((1, 1), (4, 2), (5, 2), (10, 2), (16, 8), (17, 3), (33, 4), (64, 8))


def dump(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gsmvi_amd
    K = 13
    out = {}
    for D, B in SHAPES:
        rs = np.random.RandomState(100 * D + B)
        A = rs.standard_normal((K, D, D))
        cov = A @ np.swapaxes(A, 1, 2) / D + np.eye(D)
        m = rs.standard_normal((K, D))
        X = m[:, None, :] + rs.standard_normal((K, B, D))
        G = -rs.standard_normal((K, B, D))
        tag = f"D{D}_B{B}"
        out[f"gsm_update_{tag}"] = np.concatenate([a.reshape(K, -1) for a in gsmvi_amd.gsm_update_batched(X, G, m, cov)], 1)
        out[f"bam_update_{tag}"] = np.concatenate([a.reshape(K, -1) for a in gsmvi_amd.bam_update_batched(X, G, m, cov, 2.0)], 1)
        P = np.linalg.inv(cov)
        for nan in (False, True):
            Pn = P.copy()
            if nan:
                Pn[3, 0, 0] = np.nan
            tgt = gsmvi_amd.BatchedGaussianTarget(m, precision=Pn)
            name = "nanfit" if nan else "fit"
            g = gsmvi_amd.GSMBatch(K, D, tgt.lp, tgt.lp_g)
            r = g.fit(np.arange(K), batch_size=B, niter=20, verbose=False)
            out[f"gsm_{name}_{tag}"] = np.concatenate([r[0].reshape(K, -1), r[1].reshape(K, -1), g.n_reverts[:, None]], 1)
            b = gsmvi_amd.BaMBatch(K, D, tgt.lp, tgt.lp_g)
            r = b.fit(np.arange(K), lambda i: 10.0 / (1 + i), batch_size=B, niter=20, verbose=False)
            out[f"bam_{name}_{tag}"] = np.concatenate([r[0].reshape(K, -1), r[1].reshape(K, -1), b.n_reverts[:, None]], 1)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, library {gsmvi_amd.library_path()} variant {os.environ.get('GSMVI_HIP_LIB_VARIANT', '')!r}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different contents"
    bad = [k for k in A.files if not (A[k].shape == B[k].shape and
                                      np.array_equal(A[k].view(np.uint64), B[k].view(np.uint64)))]
    print(f"{len(A.files)} arrays compared bit for bit: {len(bad)} differ {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
