# HBM bytes per launch of the preparation and of the chunk-major rescan, with and without the int8 image (tools/time_half_noi8.py):
# FETCH_SIZE and WRITE_SIZE in passes of their own (MI355X_MICROARCH.md: FETCH_SIZE doubled on gfx950) -> $OUT/summary.txt
# usage: tools/pmc_half_noi8.sh OUT_DIR      (from the repository root)
R=$PWD
[ -n "$1" ] || { echo "usage: tools/pmc_half_noi8.sh OUT_DIR"; exit 2; }
O=$R/$1
rm -rf $O && mkdir -p $O
i=0
for set in "FETCH_SIZE" "WRITE_SIZE"; do
  i=$((i+1))
  timeout -k 10 240 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $O -o p$i -- python $R/tools/time_half_noi8.py > $O/log$i.txt 2>&1 || { echo "pass $i ($set) failed"; tail -5 $O/log$i.txt; exit 1; }
  echo "pass $i ($set): ok"
done
python - $O <<'PY' > $O/summary.txt
import csv, glob, collections, sys
O = sys.argv[1]
want = ("prep_once_kernel", "match_rescan_chunk", "match_rescan_kernel", "match_gatepass", "match_refine", "match_rescore", "match_bin_survivors")
short = lambda k: k.replace("void ", "").replace("vfmm::(anonymous namespace)::", "").split("(")[0]
agg = collections.defaultdict(lambda: collections.defaultdict(list)); dur = collections.defaultdict(list)
for f in sorted(glob.glob(O + "/**/p*_counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        if any(w in r["Kernel_Name"] for w in want):
            agg[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
for f in sorted(glob.glob(O + "/**/p*_kernel_trace.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        if any(w in r["Kernel_Name"] for w in want):
            dur[short(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print("C2 (20 000 x 200 000 x 384), D.2 pair; per launch: FETCH_SIZE (KB counter; x2 on gfx950), WRITE_SIZE, duration under the counters (median)")
for k in sorted(agg):
    v = agg[k]
    f = sum(v["FETCH_SIZE"]) / max(len(v["FETCH_SIZE"]), 1); w = sum(v["WRITE_SIZE"]) / max(len(v["WRITE_SIZE"]), 1)
    dd = sorted(dur[k]); dm = dd[len(dd) // 2] if dd else float("nan")
    print(f"{k:60s} launches {len(dd):3d}  2 x FETCH_SIZE {2 * f / 1024:8.2f} MB  WRITE_SIZE {w / 1024:8.2f} MB  {dm:8.1f} us")
PY
cat $O/summary.txt
