"""Per-kernel counter sums of profiles/tools/pmc_fill.sh: python pmc_fill_parse.py OUTDIR TAG
For k_fill16 / k_est_summ: every counter summed over all launches and divided by the builds of the script (5), and the
largest single launch."""
import collections
import csv
import glob
import sys

out, tag = sys.argv[1], sys.argv[2]
BUILDS = 5
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob("%s/pmcf_%s_*/**/*counter_collection.csv" % (out, tag), recursive=True):
    for r in csv.DictReader(open(f)):
        nm = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("vr::", "")
        if nm.startswith(("k_est_summ", "k_fill16")):
            agg[nm][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k in sorted(agg):
    print("==", k)
    for c, v in sorted(agg[k].items()):
        print("  %-24s launches/build %5.1f  per build %.5g  largest launch %.5g" % (c, len(v) / BUILDS, sum(v) / BUILDS, max(v)))
