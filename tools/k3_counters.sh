#!/bin/bash
# Cache / memory-path counters of the three pipeline kernels on the headline workload (separate --pmc
# passes of a short bench run, no trace domains): L2 hits and misses, L2 <-> fabric requests, the
# vector cache's stalls, and the SQ's memory-wait split.  Run on the GPU box from the repo root:
#   tools/k3_counters.sh gpurun_out/<tag>          (EXTRA="--config 4" for the f16 pipeline)
set -o pipefail
out=${1:-gpurun_out/k3c}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
lean="--full --no-cpu-baseline --no-extra-legs --no-batch-1000 --steps 1 --warmup 1 --ramp-steps 0 --haystacks-per-step 3"
i=0
# two counters of one hardware block per pass (five TCC counters in one pass exceed what the block can
# collect: rocprofv3 aborts and then hangs), every pass under its own time limit
for set in "TCC_HIT_sum TCC_MISS_sum" "TCC_REQ_sum TCC_READ_sum" "TCC_WRITE_sum TCC_TAG_STALL_sum" \
           "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_LEVEL_sum" "TCC_EA0_RDREQ_DRAM_sum TCC_EA0_RDREQ_DRAM_CREDIT_STALL_sum" \
           "TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_STALL_sum" "TCC_EA0_WRREQ_DRAM_sum TCC_EA0_WRREQ_DRAM_CREDIT_STALL_sum" \
           "TCP_TCC_READ_REQ_sum TCP_TCC_READ_REQ_LATENCY_sum" "TCP_PENDING_STALL_CYCLES_sum TCP_GATE_EN1_sum" \
           "TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_TA_BUSY_sum" "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INST_LEVEL_VMEM SQ_INSTS_VMEM_RD"; do
  i=$((i+1))
  timeout -k 5 150 rocprofv3 --pmc $set --output-format csv -d "$out/pass$i" -o run -- python3 bench.py $lean $EXTRA > "$out/pass$i.log" 2>&1 \
    || { echo "pass $i ($set) failed or timed out" >> "$out/failed.txt"; if grep -q "caught signal" "$out/pass$i.log"; then echo "stopping: the profiler aborted" >> "$out/failed.txt"; break; fi; }
done
python3 - "$out" <<'PY'
import collections, csv, glob, json, sys
root = sys.argv[1]
KEYS = {"k1_cols_fwd": "k1_cols_fwd_", "k2_rows": ("k2_rows_r16_planes", "k2_rows_h16"), "k3_cols_inv": "k3_cols_inv_"}
vals = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{root}/pass*/**/*_counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        vals[r["Kernel_Name"]][r["Counter_Name"]].append((float(r["Counter_Value"]), int(r["Grid_Size"])))
res = {}
for key, pat in KEYS.items():
    agg = {}
    for name, counters in vals.items():
        pats = (pat,) if isinstance(pat, str) else pat
        if not any(p_ in name for p_ in pats) or name.split("(")[0].rstrip().endswith(", 1>"):   # (skip the device-side redo's K3 instantiations)
            continue
        for cname, lst in counters.items():
            gmax = max(g for _, g in lst)
            full = sorted(v for v, g in lst if g == gmax)
            agg[cname] = full[len(full) // 2]          # median over the full-size launches
    if agg:
        h, m = agg.get("TCC_HIT_sum"), agg.get("TCC_MISS_sum")
        if h is not None and m is not None and h + m > 0:
            agg["derived_l2_hit_rate"] = h / (h + m)
        def ratio(a, b):
            return agg[a] / agg[b] if agg.get(a) is not None and agg.get(b) else None
        agg["derived_fabric_read_latency_cycles"] = ratio("TCC_EA0_RDREQ_LEVEL_sum", "TCC_EA0_RDREQ_sum")
        agg["derived_l1_to_l2_read_latency_cycles"] = ratio("TCP_TCC_READ_REQ_LATENCY_sum", "TCP_TCC_READ_REQ_sum")
        agg["derived_share_of_fabric_reads_from_dram"] = ratio("TCC_EA0_RDREQ_DRAM_sum", "TCC_EA0_RDREQ_sum")
        agg["derived_vmem_in_flight_per_wave_cycle"] = ratio("SQ_INST_LEVEL_VMEM", "SQ_WAVE_CYCLES")
        res[key] = agg
json.dump(res, open(f"{root}/cache_counters.json", "w"), indent=1)
print(json.dumps(res, indent=1))
PY
find "$out" -maxdepth 1 -type d -name "pass*" -exec rm -rf {} +
echo collected
