"""Per-launch HBM bytes of the bench's dominant kernel classes from the two rocprofv3 PMC passes.

gfx950 corrections (MI355X_MICROARCH.md §HBM): FETCH_SIZE (KB) counts exactly half of the bytes of a
16-B/lane coalesced streaming read -> x2 (our GEMM operands are float4 loads); WRITE_SIZE (KB) is exact
for 16-B/lane stores, which is what the GEMM epilogues issue (float4 runs of the C^T tile).
Writes profiles/traffic.json {class: bytes per launch} for the fine-net trunk launches (M = 786,432)."""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

root = sys.argv[1]
M_FINE = 4096 * 192
CLASSES = {
    "fwd": ("gemm_nt16_kernel<128, 128, 2, 1,", 0),
    "dgrad": ("gemm_nt16_kernel<128, 128, 2, 2,", 0),
    "wgrad": ("gemm_wgrad_kernel<128, 128, 2,", 0),
}
if len(sys.argv) > 2 and sys.argv[2] == "bf16fused":  # the fused bf16 MLP (bench.py roofline_bf16 classes)
    CLASSES = {
        "fused_bwd_layer": ("bwd_layer_bf16_kernel", 0),
        "fused_fwd": ("mlp_fwd_fused_bf16_kernel<true", 0),
    }
elif len(sys.argv) > 2 and sys.argv[2] == "bf16":  # layered bf16 MLP (configs[2]) kernel names
    CLASSES = {
        "fwd": ("gemm_nt_bf16_wsr_kernel<256, 128, 1, 1,", 0),
        "dgrad": ("gemm_nt_bf16_wsr_kernel<256, 128, 2, 1,", 0),
        "wgrad": ("gemm_wgrad_bf16_kernel<128, 128, 2,", 0),
    }


def load(counter):
    files = glob.glob(os.path.join(root, counter, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no counter_collection.csv under {root}/{counter}")
    rows = list(csv.DictReader(open(files[0])))
    return rows


def per_kernel(rows):
    out = defaultdict(list)
    for r in rows:
        name = r.get("Kernel_Name") or r.get("Kernel-Name") or ""
        grid = int(float(r.get("Grid_Size") or r.get("Grid_Size_X") or 0))
        val = float(r.get("Counter_Value") or 0)
        out[(name, grid)].append(val)
    return out


def upper(vals):
    if not vals:
        return vals
    cut = 0.5 * (max(vals) + min(vals))
    return [v for v in vals if v >= cut] if max(vals) > 1.5 * min(vals) else vals


fetch = per_kernel(load("FETCH_SIZE"))
write = per_kernel(load("WRITE_SIZE"))
if len(sys.argv) <= 2 and any("_x6" in k[0] for k in fetch):  # fp32 split-product GEMMs (gemm_x6.hpp)
    split_dgrad = any("gemm_nt_x6w_kernel<2," in k[0] for k in fetch)
    CLASSES = {
        # one launch per layer: only with NERF_MLP_FWD_LAYERED or events (bench.py --full's roofline pass); the plain
        # bench runs the whole trunk of a net in one gemm_nt_x6w_chain_kernel launch ("fwd_chain": bytes of 8 layers)
        "fwd": ("gemm_nt_x6w_kernel<1,", 0),
        "fwd_chain": ("gemm_nt_x6w_chain_kernel", 0),
        # default engine: the split input-gradient kernel (small-term accumulators); NERF_MLP_NATIVE_DGRAD: fp32 16x16x4
        "dgrad": ("gemm_nt_x6w_kernel<2," if split_dgrad else "gemm_nt16_kernel<128, 128, 2, 2,", 0),
        # the plain bench runs the seven input gradients of a net in one gemm_nt_x6w_dgrad_chain_kernel launch
        # ("dgrad_chain": bytes of 7 layers); the per-layer class above appears with NERF_MLP_BWD_LAYERED or events
        "dgrad_chain": ("gemm_nt_x6w_dgrad_chain_kernel", 0),
        "wgrad": ("gemm_wgrad_x6w_kernel", 0),
    }
res, detail = {}, {}
for cls, (pat, _) in CLASSES.items():
    # the fine-net trunk launches are the ones with the largest grid of that kernel
    keys = [k for k in fetch if pat in k[0]]
    if not keys:
        print(f"pmc_parse: no launch of class {cls!r} ({pat}) in this run", file=sys.stderr)
        continue
    gmax = max(k[1] for k in keys)
    kf = [k for k in keys if k[1] == gmax]
    # the persistent bf16 kernels launch a fixed grid for both nets: keep the fine-net launches, which
    # move 3x the bytes of the coarse ones (M = 786,432 vs 262,144), by the upper cluster of the values
    fvals = upper([v for k in kf for v in fetch[k]])
    wvals = upper([v for k in kf for v in write.get(k, [])])
    fb = 2.0 * 1024 * sum(fvals) / len(fvals)
    wb = 1024 * sum(wvals) / max(1, len(wvals))
    calib = 1.0  # the epilogues store 16 B per lane: WRITE_SIZE is exact for that width (MI355X_MICROARCH.md)
    res[cls] = round(fb + wb * calib)
    detail[cls] = {"fetch_bytes_x2": round(fb), "write_bytes_raw": round(wb), "write_calib": round(calib, 3),
                   "launches": len(fvals), "grid": gmax}
print(json.dumps(detail, indent=1))
json.dump(res, open(os.path.join(root, "traffic.json"), "w"), indent=1)  # copy to profiles/ after the run
json.dump(detail, open(os.path.join(root, "traffic_detail.json"), "w"), indent=1)
print(json.dumps(res))
