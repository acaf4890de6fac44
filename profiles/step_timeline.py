#!/usr/bin/env python3
"""Per-step timeline of the read loop from a `rocprofv3 --kernel-trace --output-format csv` run of bench.py.

    python3 profiles/step_timeline.py <directory with *_kernel_trace.csv> [steps]

For each of the last `steps` (default 20) main-tier wave-kernel dispatches: where the counter reset (a fill kernel), the pack
kernel and the wave kernel start and end, relative to the end of the wave kernel before; the gaps between them on the main
stream; and where the previous batch's deep tier and vg_late_collect fall.  All times in microseconds."""
import csv
import glob
import os
import re
import statistics
import sys

src = sys.argv[1]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
files = glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
assert files, "no *kernel_trace.csv under %s" % src
rows = []
for f in files:
    for r in csv.DictReader(open(f)):
        rows.append({"name": r["Kernel_Name"], "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]), "q": r.get("Queue_Id", "?"), "wg": r.get("Workgroup_Size", r.get("Workgroup_Size_X", "?"))})
rows.sort(key=lambda r: r["s"])


def kind(r):
    n = r["name"]
    if "vg_pack_kernel" in n:
        return "pack"
    if "vg_late_collect" in n:
        return "late"
    if "vg_wave_kernel" in n:
        return "wave" if re.search(r", 4(, (false|true))?>", n) else "deep"
    if "fillBuffer" in n:
        return "fill"
    return "other"


for r in rows:
    r["k"] = kind(r)
waves = [r for r in rows if r["k"] == "wave"]
assert len(waves) > steps, "%d main-tier dispatches in the trace, %d steps asked for" % (len(waves), steps)
main_q = waves[-1]["q"]
all_packs = [r for r in rows if r["k"] == "pack"]
us = lambda ns: ns / 1e3
out = ["# %s: the last %d of %d main-tier dispatches; main stream's queue %s; microseconds, t = 0 at the end of the wave kernel before" % (os.path.basename(files[0]), steps, len(waves), main_q),
       "# step | reset: queue start end | pack: queue start end dur | wave: start end dur | idle on the main stream: prev wave->first, reset->pack, pack->wave, sum | step = wave end | deep tier of the batch before: queue start end | late_collect end | reset on another queue: queue start end"]
acc = {k: [] for k in ("pack", "wave", "g0", "g1", "g2", "idle", "step", "deep_s", "deep_e", "fill_main")}
for i in range(len(waves) - steps, len(waves)):
    w, pw = waves[i], waves[i - 1]
    t0 = pw["e"]
    # a batch has one pack and one wave dispatch: the i-th of each belong together (a pack kernel on the ingest stream may start
    # anywhere inside the wave kernel before); a trace with packed batches in it falls back to "the last pack before this wave"
    packs = [r for r in rows if r["k"] == "pack" and pw["s"] < r["s"] < w["s"]]
    p = all_packs[i] if len(all_packs) == len(waves) else (packs[-1] if packs else None)
    # the reset that belongs to this batch when it is on the pack kernel's queue: the last fill before the pack kernel on that queue
    fills = [r for r in rows if r["k"] == "fill" and p and r["q"] == p["q"] and p["s"] - 100000 < r["s"] < p["s"]]
    fl = fills[-1] if fills else None
    # ... and a reset on another queue (the tail stream's, behind the tiers of the batch before): the last one inside this step
    ofills = [r for r in rows if r["k"] == "fill" and r["q"] != main_q and (not p or r["q"] != p["q"]) and pw["e"] < r["s"] <= w["e"]]
    ofl = ofills[-1] if ofills else None
    deep = [r for r in rows if r["k"] == "deep" and pw["s"] < r["s"] <= w["e"]]
    late = [r for r in rows if r["k"] == "late" and pw["s"] < r["s"] <= w["e"]]
    on_main = [x for x in (fl, p) if x and x["q"] == main_q]
    g0 = (on_main[0]["s"] if on_main else w["s"]) - t0                       # previous wave kernel's end -> first dispatch of this batch on the main stream
    g1 = (p["s"] - fl["e"]) if (fl and p and fl["q"] == main_q and p["q"] == main_q) else 0
    g2 = (w["s"] - max(p["e"], t0)) if p else 0
    if p and p["q"] != main_q:                                               # the pack kernel ran on another stream: the main stream idles from wave to wave
        g0, g1, g2 = w["s"] - t0, 0, 0
    idle = max(g0, 0) + max(g1, 0) + max(g2, 0)
    f = lambda r, keys: " ".join(("%8.1f" % us(r[k] - t0)) for k in keys) if r else " ".join(["       -"] * len(keys))
    out.append("%4d | %3s %s | %3s %s %7.1f | %s %7.1f | %6.1f %6.1f %6.1f %6.1f | %8.1f | %3s %s | %s | %3s %s" % (
        i - (len(waves) - steps), fl["q"] if fl else "-", f(fl, ("s", "e")), p["q"] if p else "-", f(p, ("s", "e")), us(p["e"] - p["s"]) if p else 0.0,
        f(w, ("s", "e")), us(w["e"] - w["s"]), us(g0), us(g1), us(g2), us(idle), us(w["e"] - t0),
        deep[0]["q"] if deep else "-", f({"s": min(r["s"] for r in deep), "e": max(r["e"] for r in deep)} if deep else None, ("s", "e")), f(late[-1] if late else None, ("e",)), ofl["q"] if ofl else "-", f(ofl, ("s", "e"))))
    if p:
        acc["pack"].append(us(p["e"] - p["s"]))
    acc["wave"].append(us(w["e"] - w["s"])); acc["g0"].append(us(g0)); acc["g1"].append(us(g1)); acc["g2"].append(us(g2)); acc["idle"].append(us(idle)); acc["step"].append(us(w["e"] - t0))
    if fl and fl["q"] == main_q:
        acc["fill_main"].append(us(fl["e"] - fl["s"]))
    if deep:
        acc["deep_s"].append(us(min(r["s"] for r in deep) - t0)); acc["deep_e"].append(us(max(r["e"] for r in deep) - t0))
md = lambda v: statistics.median(v) if v else float("nan")
out.append("# medians: pack %.1f  wave %.1f  step (wave end to wave end) %.1f  idle on the main stream %.1f = prev wave->first %.1f + reset->pack %.1f + pack->wave %.1f;  reset kernel on the main stream %.1f (n=%d);  deep tier of the batch before runs %.1f .. %.1f" % (
    md(acc["pack"]), md(acc["wave"]), md(acc["step"]), md(acc["idle"]), md(acc["g0"]), md(acc["g1"]), md(acc["g2"]), md(acc["fill_main"]), len(acc["fill_main"]), md(acc["deep_s"]), md(acc["deep_e"])))
out.append("# pack dispatches that run inside the span of a wave kernel (start or end between a wave kernel's start and end): %d of %d" % (sum(1 for r in all_packs[len(all_packs) - steps:] if any(x["s"] < r["s"] < x["e"] or x["s"] < r["e"] < x["e"] for x in waves)), steps))
print("\n".join(out))
