#!/usr/bin/env python3
"""Time the multi-vector apply (mas_apply_multi_device) against single applies.

For each configuration (default: the bench configuration 1M + contacts, and
256k) and each K in {1, 2, 4, 8}: one batched apply of K residuals against K
single applies of the same residuals, on the same handle in the same process,
interleaved -- per repeat, HIP events around N back-to-back batched calls, then
around N x K back-to-back single calls, after a warm-up of both; the median
over the repeats is kept.  Before timing, the batch's z is checked bit for bit
against the single applies.

Writes profiles/multi_rhs/<config>.json: ms per batch, ms per vector, the
ratio to K interleaved single applies, the algorithmic bytes of the batch (the
inverses once per pass of up to 4 vectors, 16 B of map per vertex and pass,
32 B of r and z per vertex and vector) and their fraction of the 8 TB/s HBM
peak.  Needs a GPU; there is no fallback.

    python scripts/multi_rhs_time.py [--configs 1M+contacts 256k] [--calls 200] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "preconditioner-for-cloth-and-deformable-body-simulation_amd", "python"))

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E spec
BLOCK_BYTES = 4656 * 4     # fp32 packed inverse
NARROW_BYTES = 14272       # its 24-bit copy (csrc/narrow.h)
PASS_K = 4                 # vectors per pass over the inverses (csrc/k_multi.hip)


def batch_bytes(info, K, wide):
    """Algorithmic bytes of one batched apply of K vectors."""
    passes = -(-K // PASS_K)
    nV, fine, blocks = info["num_verts"], info["num_fine_blocks"], info["num_blocks"]
    inv = fine * (BLOCK_BYTES if wide else NARROW_BYTES) + (blocks - fine) * BLOCK_BYTES
    return passes * (inv + nV * 16) + K * nV * 32


def time_config(name, calls, repeats, warmup, wide):
    import numpy as np
    import torch
    import mas_amd
    from mas_amd import meshgen
    mesh, cfg = meshgen.build_config(name)
    contacts = meshgen.vf_contacts(mesh, cfg["contacts"], seed=3) if cfg["contacts"] else None
    P = mas_amd.from_mesh(mesh, max_levels=cfg["levels"], contacts=contacts, wide_inverse=wide)
    info = P.info()
    nV, KMAX = mesh.nV, 8
    r = torch.from_numpy(np.stack([meshgen.residual(nV, 0x5EED + k) for k in range(KMAX)])).cuda()
    zb = torch.zeros_like(r)
    zs = torch.zeros_like(r)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    torch.cuda.synchronize()

    def batched(K):
        P.PreconditioningDeviceMulti(zb[:K], r[:K], sp)

    def singles(K):
        for k in range(K):
            P.PreconditioningDevice(zs[k], r[k], sp)

    def timed(fn, K, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn(K)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    out = {"config": name, "num_verts": nV, "num_levels": int(info["num_levels"]),
           "num_fine_blocks": int(info["num_fine_blocks"]), "num_blocks": int(info["num_blocks"]),
           "wide_inverse": bool(wide), "calls_per_repeat": calls, "repeats": repeats, "warmup": warmup,
           "hbm_peak_bytes_per_s": HBM_PEAK, "K": {}}
    for K in (1, 2, 4, 8):
        batched(K)
        singles(K)
        stream.synchronize()
        if not np.array_equal(zb[:K].cpu().numpy().view(np.uint32), zs[:K].cpu().numpy().view(np.uint32)):
            raise SystemExit(f"{name} K={K}: the batch is not bitwise the single applies")
        for _ in range(warmup):
            batched(K)
            singles(K)
        stream.synchronize()
        tb, ts = [], []
        for _ in range(repeats):
            tb.append(timed(batched, K, calls))
            ts.append(timed(singles, K, calls))
        mb, ms = statistics.median(tb), statistics.median(ts)
        nbytes = batch_bytes(info, K, wide)
        out["K"][str(K)] = {
            "batch_ms": mb, "batch_ms_min": min(tb), "batch_ms_max": max(tb),
            "per_vector_ms": mb / K,
            "k_single_applies_ms": ms, "single_apply_ms": ms / K,
            "ratio_to_k_single_applies": mb / ms,
            "batch_in_single_applies": mb / (ms / K),
            "algorithmic_bytes": nbytes,
            "fraction_of_hbm_peak": nbytes / (mb * 1e-3) / HBM_PEAK,
        }
        print(f"{name} K={K}: batch {mb * 1e3:.1f} us ({mb / K * 1e3:.1f} us/vector), {K} single applies "
              f"{ms * 1e3:.1f} us, batch = {mb / (ms / K):.2f} single applies, "
              f"{nbytes / 1e6:.0f} MB = {out['K'][str(K)]['fraction_of_hbm_peak'] * 100:.0f} % of 8 TB/s",
              file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["1M+contacts", "256k"])
    ap.add_argument("--calls", type=int, default=200, help="back-to-back calls between two events")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--wide-inverse", action="store_true", help="time the fp32 inverses instead of the 24-bit copy")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multi_rhs"))
    args = ap.parse_args()
    if args.calls < 1 or args.repeats < 1:
        ap.error("--calls and --repeats must be positive")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_rhs_time.py needs a GPU")
    os.makedirs(args.out, exist_ok=True)
    for name in args.configs:
        res = time_config(name, args.calls, args.repeats, args.warmup, args.wide_inverse)
        path = os.path.join(args.out, name.replace("+", "_") + ".json")
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(path)


if __name__ == "__main__":
    main()
