#!/bin/bash
# Counter passes over the pack kernel and the unpack kernel of cfg 2's shape (8192 x 5464, 14-bit
# MSB), each pass a run of its own with nothing else traced:  scripts/pmc_encode_pack.sh OUT_DIR
# Writes OUT_DIR/set<i>.csv and OUT_DIR/summary.txt: per kernel and counter the mean over the
# launches.  Read against each other the two kernels show where the pack kernel's time goes:
# loads and stores issued a wavefront, vector-ALU instructions a wavefront, the share of the
# wavefronts' cycles spent waiting, the bytes fetched and written.
set -u
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$REPO/profiles/encode/pmc}
mkdir -p "$OUT"
TMP=$(mktemp -d)
i=0
for set in "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR" \
           "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" \
           "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --pmc $set --output-format csv -d "$TMP/p$i" -- \
    python "$REPO/bench_encode.py" --pmc-leg > /dev/null 2>&1 || { echo "pass $i failed"; exit 1; }
  cp "$(find "$TMP/p$i" -name '*counter_collection.csv' | head -1)" "$OUT/set$i.csv" || exit 1
done
python - "$OUT" > "$OUT/summary.txt" <<'PY'
import collections, csv, glob, sys
acc = collections.defaultdict(list)
for path in sorted(glob.glob(sys.argv[1] + "/set*.csv")):
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"]
        kernel = "encode_pack_kernel" if "encode_pack_kernel" in n else "unpack_kernel" if "unpack_kernel" in n else None
        if kernel:
            acc[(kernel, r["Counter_Name"])].append(float(r["Counter_Value"]))
for (kernel, counter), v in sorted(acc.items()):
    print("%-20s %-22s %16.1f  (%d launches)" % (kernel, counter, sum(v) / len(v), len(v)))
PY
cat "$OUT/summary.txt"
rm -rf "$TMP"
