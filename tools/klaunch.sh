#!/bin/bash
# LAUNCH PARAMETERS of every kernel of a run (rocprofv3 --kernel-trace), sibling of tools/kseq.sh: name, grid, workgroup and LDS bytes.
#   bash tools/klaunch.sh OUT NAME step -- python3 bench.py --config cfg5 --no-cpu-baseline --no-extras --steps 3 --warmup 1
#       the launches between the last two step-closing kernels, in order              -> OUT/kl_NAME.txt
#   bash tools/klaunch.sh OUT NAME set -- python3 -m pytest tests/test_gpu_pair_sweep_bits.py -q
#       the sorted set of distinct (kernel, grid, workgroup, LDS) tuples of the run   -> OUT/kl_NAME.txt
# Two libraries launch alike when the files of two runs (LGN_AMD_LIB selects the library) are identical.
OUT=$1; NAME=$2; MODE=$3; shift; shift; shift; shift
ROOT=$(pwd); mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
ARGS=(); for x in "$@"; do if [ -e "$ROOT/$x" ]; then ARGS+=("$ROOT/$x"); else ARGS+=("$x"); fi; done
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv -d "$OUT/kl_$NAME" -- "${ARGS[@]}" > "$OUT/kl_$NAME.log" 2>&1 || { tail -20 "$OUT/kl_$NAME.log"; exit 1; }
cd "$ROOT"
python3 - "$OUT/kl_$NAME" "$MODE" > "$OUT/kl_$NAME.txt" <<'PY' || exit 1
import csv, glob, sys
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):      # (pytest: one file per process that used the GPU)
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
lds = next(k for k in rows[0] if "lds" in k.lower())         # LDS_Block_Size in the rocprofv3 this was written with
tup = lambda r: (r["Kernel_Name"], "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"), r[lds])
fmt = lambda t: f"{t[1]:>16s} {t[2]:>10s} {t[3]:>7s}  {t[0][:160]}"
if sys.argv[2] == "step":
    idx = [i for i, r in enumerate(rows) if "l1_adam" in r["Kernel_Name"] or "step_tail" in r["Kernel_Name"]]
    sel = [tup(r) for r in rows[idx[-2] + 1:idx[-1] + 1]]
    print(f"# {len(sel)} launches of one step: grid, workgroup, {lds}, kernel")
else:
    sel = sorted(set(tup(r) for r in rows))
    print(f"# {len(sel)} distinct launches of {len(rows)}: grid, workgroup, {lds}, kernel")
print("\n".join(fmt(t) for t in sel))
PY
rm -rf "$OUT/kl_$NAME"
tail -n 3 "$OUT/kl_$NAME.txt"
