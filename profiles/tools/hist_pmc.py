"""What bounds k_hist_bricks: hardware counters, taken in runs of their own (no timing in them):
python profiles/tools/hist_pmc.py [--out FILE]

Starts itself as a child under rocprofv3 --pmc once per counter set (a counter set is what one pass can collect).  The
child calls vr_histogram_bricks twice on each of three 2 GiB buffers of 256 bricks -- uniform random bytes, the bench's
mix (4096-byte runs, two thirds of them constant) and one constant value -- and once more on the random buffer without
the data-aware paths (vr_debug_set "hist_plain").  The parent reads the counter files, keeps the second call on each
buffer and writes, per buffer, the counters and the shares that say where the waves' cycles go.
Writes the report to profiles/hist_pmc.txt (or --out)."""
import argparse
import collections
import csv
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SETS = [["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"],
        ["SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_ACTIVE_INST_VMEM", "SQ_ACTIVE_INST_SCA"],
        ["SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_SALU"],
        ["SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_WAIT_INST_LDS", "SQ_WAVES"]]
CALLS = ["random (warm-up)", "random", "mix (warm-up)", "mix", "constant (warm-up)", "constant", "random, plain"]


def work():
    sys.path.insert(0, ROOT)
    import torch
    import volumerenderer_amd as vr
    from volumerenderer_amd import _lib
    n, B = 1 << 31, 256
    rnd = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    blocks = n // 4096
    keep = torch.rand(blocks, device="cuda") >= 2.0 / 3.0
    fill = torch.randint(0, 256, (blocks, 1), dtype=torch.uint8, device="cuda").expand(blocks, 4096)
    mix = torch.where(keep[:, None], rnd.reshape(blocks, 4096), fill).reshape(-1).contiguous()
    const = torch.full((n,), 37, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for buf in (rnd, mix, const):
        for _ in range(2):
            vr.histogram_bricks(buf, B)
    assert _lib.lib().vr_debug_set(b"hist_plain", 1) == 0
    vr.histogram_bricks(rnd, B)
    assert _lib.lib().vr_debug_set(b"hist_plain", 0) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_pmc.txt"))
    ap.add_argument("--work", action="store_true")
    args = ap.parse_args()
    if args.work:
        return work()
    per_call = collections.defaultdict(dict)          # call index -> counter -> value summed over the device
    for counters in SETS:
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run(["rocprofv3", "--pmc", *counters, "--output-format", "csv", "-d", d, "--", sys.executable,
                                os.path.abspath(__file__), "--work"], capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                print("pass failed:", " ".join(counters), (r.stdout + r.stderr)[-400:], flush=True)
                continue
            rows = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                rows += [x for x in csv.DictReader(open(f)) if "k_hist_bricks" in x["Kernel_Name"]]
            ids = sorted({int(x["Dispatch_Id"]) for x in rows})
            for x in rows:
                c = per_call[ids.index(int(x["Dispatch_Id"]))]
                c[x["Counter_Name"]] = c.get(x["Counter_Name"], 0.0) + float(x["Counter_Value"])
    lines = ["k_hist_bricks, 2 GiB as 256 bricks, counters summed over the device, one rocprofv3 --pmc pass per row of counters"]
    for i, name in enumerate(CALLS):
        if "warm-up" in name or i not in per_call:
            continue
        c = per_call[i]
        lines.append("== %s" % name)
        for counters in SETS:
            lines.append("  " + "  ".join("%s %.4g" % (k, c[k]) for k in counters if k in c))
        wc = c.get("SQ_WAVE_CYCLES")
        if wc:
            share = lambda k: 100.0 * c.get(k, 0.0) / wc      # noqa: E731
            lines.append("  of the waves' cycles: LDS instructions active %.1f %%, waiting on LDS %.1f %%, VALU active %.1f %%, "
                         "VMEM active %.1f %%, waiting on anything %.1f %%"
                         % (share("SQ_ACTIVE_INST_LDS"), share("SQ_WAIT_INST_LDS"), share("SQ_ACTIVE_INST_VALU"),
                            share("SQ_ACTIVE_INST_VMEM"), share("SQ_WAIT_INST_ANY")))
        if c.get("SQ_LDS_IDX_ACTIVE"):
            lines.append("  LDS bank-conflict cycles per LDS index cycle: %.2f; LDS instructions per VALU instruction: %.2f"
                         % (c.get("SQ_LDS_BANK_CONFLICT", 0.0) / c["SQ_LDS_IDX_ACTIVE"], c.get("SQ_INSTS_LDS", 0.0) / max(1.0, c.get("SQ_INSTS_VALU", 0.0))))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
