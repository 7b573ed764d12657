"""HBM traffic and clock per kernel from rocprofv3 --pmc passes over bench.py -> profiles/pmc_traffic.json.

    python tools/pmc_traffic.py <prof_dir> [out.json]

<prof_dir>/fetch, /write, /clock hold the counter_collection CSVs of three separate passes
(tools/profile_round.sh).  Per the gfx950 notes of the MI355X guide: FETCH_SIZE (KB) counts half the
bytes of 16-B-per-lane streaming reads (glds included) -> doubled; WRITE_SIZE (KB) is exact for
16-B stores.  hbm_bytes_per_launch = (2*FETCH_SIZE + WRITE_SIZE) * 1024, mean over the dispatches.
Effective clock = GRBM_GUI_ACTIVE / 8 XCDs / kernel duration.  Keys are bench.py's kernel tags.
The output names the build id of the library the passes ran (pu_build_id()); bench.py reports
roofline.traffic only when that id equals the id of the library it is running.
"""
import collections
import csv
import glob
import json
import os
import re
import sys


def tag_of(name, grid=None):
    # the Winograd kernels: bench.py tags unsplit launches igemm<256x64,wino> (grid 256 x 512
    # threads, persistent or one block per item) and split-K ones with ",k<n>" (fewer items)
    if "wgrad_wino_cols_x6_kernel" in name:
        return "wgrad<128x384,wino,x6>"
    if "wgrad_wino_x6_kernel" in name:
        return "wgrad<64x576,wino,x6>"
    if "wino_x6_kernel" in name:
        return "igemm<256x64,wino>" if grid is None or int(grid) >= 131072 else "igemm<256x64,wino,split>"
    if "igemm_bf16_rows_kernel" in name:
        return "igemm_bf16<128x64,rows>"
    m = re.search(r"igemm_bf16_halo_kernel<(\d+)>", name)
    if m:
        return "igemm_bf16<256x64,halo>"
    m = re.search(r"igemm_bf16_lean_kernel<(\d+), (\d+),", name)
    if m:
        return "igemm_bf16<%sx%s,lean>" % m.groups()
    m = re.search(r"wgrad_halo_bf16_kernel<(\d)>", name)
    if m:
        return "wgrad_bf16<%dx576,halo>" % (64 * int(m.group(1)))
    if "wgrad_halo_x6_kernel<2>" in name:
        return "wgrad<128x576,halo,x6>"
    if "wgrad_halo_x6_kernel" in name:
        return "wgrad<64x576,halo,x6>"
    m = re.search(r"igemm_x6_lean_kernel<(\d+), (\d+),", name)
    if m:
        return "igemm<%sx%s,x6>" % m.groups()
    m = re.search(r"wgrad_dma_kernel<(\d+), (\d+), \d+, \d+, \d+, (true|false)[,>]", name)
    if m:
        return "wgrad<%sx%s,vec4%s>" % (m.group(1), m.group(2), ",x6" if m.group(3) == "true" else "")
    m = re.search(r"igemm_x6_kernel<(\d+), (\d+),", name)
    if m:
        return "igemm<%sx%s,x6>" % m.groups()
    m = re.search(r"wgrad_dma_kernel<(\d+), (\d+),", name)
    if m:
        return "wgrad<%sx%s,vec4>" % m.groups()
    m = re.search(r"wgrad_kernel<(\d+), (\d+), \d+, \d+, (true|false)>", name)
    if m:
        return "wgrad<%sx%s,%s>" % (m.group(1), m.group(2), "vec4" if m.group(3) == "true" else "scalar")
    m = re.search(r"igemm_dma_kernel<(\d+), (\d+),", name)
    if m:
        return "igemm<%sx%s,chunk16>" % m.groups()
    m = re.search(r"igemm_kernel<(\d+), (\d+), \d+, \d+, (\d)>", name)
    if m:
        return "igemm<%sx%s,%s>" % (m.group(1), m.group(2), ("chunk16", "vec4", "scalar")[int(m.group(3))])
    m = re.search(r"pu::(\w+?)(_kernel)?[<(]", name)
    return m.group(1) if m else name


def load(d):
    """-> {tag: {counter: [per-dispatch values]}}, {tag: [durations ns]}"""
    vals = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        per = collections.defaultdict(float)
        names = {}
        for r in csv.DictReader(open(f)):
            key = (r.get("Dispatch_Id") or r.get("Correlation_Id"), r["Counter_Name"])
            per[key] += float(r["Counter_Value"])      # summed over dimensions (XCD/SE instances)
            names[key[0]] = (r.get("Kernel_Name", "?"), r.get("Grid_Size"))
        for (disp, cn), v in per.items():
            vals[tag_of(*names[disp])][cn].append(v)
    durs = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            grid = r.get("Grid_Size") or r.get("Grid_Size_X")
            durs[tag_of(r["Kernel_Name"], grid)].append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    return vals, durs


def main():
    d = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/pmc_traffic.json"
    fetch, _ = load(os.path.join(d, "fetch"))
    write, _ = load(os.path.join(d, "write"))
    clock, cdur = load(os.path.join(d, "clock"))
    res = {}
    for tag in sorted(set(fetch) | set(write)):
        f = fetch.get(tag, {}).get("FETCH_SIZE", [])
        w = write.get(tag, {}).get("WRITE_SIZE", [])
        if not f or not w:
            continue
        mf, mw = sum(f) / len(f), sum(w) / len(w)
        e = {"dispatches": len(f), "fetch_size_kb_raw": round(mf, 1), "write_size_kb": round(mw, 1),
             "hbm_bytes_per_launch": round((2 * mf + mw) * 1024.0)}
        g = clock.get(tag, {}).get("GRBM_GUI_ACTIVE", [])
        ds = cdur.get(tag, [])
        if g and ds:
            e["effective_clock_ghz"] = round(sum(g) / len(g) / 8.0 / (sum(ds) / len(ds)), 3)
        mb = clock.get(tag, {}).get("SQ_VALU_MFMA_BUSY_CYCLES", [])
        if mb and g:
            # MFMA-busy cycles summed over all SIMDs vs wall cycles x 1024 SIMDs
            e["mfma_busy_frac"] = round((sum(mb) / len(mb)) / ((sum(g) / len(g)) / 8.0 * 1024), 4)
        res[tag] = e
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plastic-unet_amd"))
    from punet import _lib
    json.dump({"build_id": _lib.build_id(), "kernels": res}, open(out, "w"), indent=1, sort_keys=True)
    for k, v in res.items():
        print("%-28s %s" % (k, v))


if __name__ == "__main__":
    main()
