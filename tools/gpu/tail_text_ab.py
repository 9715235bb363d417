#!/usr/bin/env python3
"""SAM text on the host against SAM text on the device (BM2_SAM_F_DEVICE_TEXT), on ONE chunk with nothing else running: the device
produces the hits of a paired chunk once (the bench's cached genome), then bm2_sam_pe_dev runs on it with the bit off and on, ALTERNATING
in one process -- two warm-up calls each, then --calls timed calls each, the two texts compared every time.  Per variant: median and
spread of wall ms and of process CPU-s per call (resource.getrusage), the phases BM2_TAIL_PROF=1 prints (medians), the counters of
bm2_sam_text_stats and the bytes that cross PCIe each way, counted from the chunk.  --parent-lib: a second process of this tool loads
that library (the parent commit's build) and times its bit-off path on the same chunk first: the baseline for "CPU-s per chunk".
    python tools/gpu/tail_text_ab.py --out profiles/sam_text_dev_ab.json [--parent-lib PATH] [--pairs 500000] [--genome-mbp 3100] [--calls 10]
--bit text|decide|both: which opt-in bit the "on" variant sets (BM2_SAM_F_DEVICE_TEXT, BM2_SAM_F_DEVICE_DECIDE: the pairs' decisions from
bm2_pe_decide_dev, or the two together); with decide the result also holds bm2_sam_decide_stats and the bytes the decisions move.
--bit rescue|rescue+decide|all: BM2_SAM_F_DEVICE_RESCUE (the mate-rescue results applied by bm2_pe_rescue_apply_dev's kernels) alone, with
the decide bit, with both others; the result then holds bm2_sam_rescue_apply_stats and the bytes the lists and tasks move.
--bit plan|plan+rescue|plan+rescue+decide+text: BM2_SAM_F_DEVICE_PLAN (mate rescue planned by bm2_pe_rescue_plan_dev's kernels, the rescue
batch's queries made on the device) alone, with the rescue bit, with all three others; the result then holds bm2_sam_rescue_plan_stats and
the bytes the plan and the queries move.
--bit pestat|pestat+plan: BM2_SAM_F_DEVICE_PESTAT (the chunk's insert-size model counted by bm2_pe_stat_dev's kernel) alone and with the
plan bit, which then reads the hits where the model left them; the result holds bm2_sam_pestat_stats and the bytes the model moves.  The
phases to read: `sam_pe: pestat` against `sam_pe: pestat (device)`, and `pe_plan_dev: H2D` of --bit plan against --bit pestat+plan.
--bit cgplan|all+cgplan: BM2_SAM_F_DEVICE_CGPLAN (the CIGAR batch picked by bm2_cigar_plan_dev's kernels, no dry emit pass) alone and with
the five other bits; the result holds bm2_sam_cigar_plan_stats and the bytes the plan moves.  The phases to read: `sam_pe: decide + dry
emit` against `sam_pe: decide` + `sam_pe: cigar plan (device)`, and `cigar_session: batch list`.
--bit semark|semark+cgplan (these imply --single-end): BM2_SAM_F_DEVICE_SEMARK (the single-end tail's primary hits marked by
bm2_se_mark_dev's kernels, one call a chunk) alone and with the CIGAR plan reading the marked lists where they lie; the result holds
bm2_sam_se_mark_stats and the bytes the marking moves.  The phases to read: `sam_se: decide` against `sam_se: decide (device)`.
--bit cgprep|all+cgplan+cgprep|semark+cgplan+cgprep (the last implies --single-end): BM2_SAM_F_DEVICE_CGPREP (the CIGAR batch's task slices
and class order made by bm2_cigar_prep_dev's kernels where the batch runs) alone and with every other bit of the paired / single-end tail;
the result holds bm2_sam_cigar_prep_stats and the bytes the preparation moves.  The phases to read: `gen_cigar_dev: slices` +
`gen_cigar_dev: order` against `gen_cigar_dev: prep (device)`.
--single-end: the two files of the chunk as ONE single-end input of 2 x --pairs reads through bm2_sam_se_dev (any bit the single-end tail takes).
--once: one bit-on call and nothing else (what a kernel trace of k_sam_size / k_sam_write is taken from)."""
import argparse
import json
import os
import re
import resource
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bwa-mem2_amd"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
os.environ.setdefault("BM2_MALLOC_TUNE", "1")


def cpu_s():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


class Stderr:
    """fd 2 into a file while the library prints its phases"""

    def __enter__(self):
        self.f = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read().decode(errors="replace")
        self.f.close()


def phases(text):
    out = {}
    for m in re.finditer(r"\[tail\] (\S+)\s+(.+?)\s+([0-9.]+) ms", text):
        out.setdefault("%s: %s" % (m.group(1), m.group(2).strip()), []).append(float(m.group(3)))
    return {k: sum(v) for k, v in out.items()}


def spread(v):
    v = sorted(v)
    return {"median": float(np.median(v)), "min": v[0], "max": v[-1], "n": len(v)}


def pcie_ledger(text, n_reads, name_bytes, host_blob):
    """bytes the device-text path moves, counted from the chunk's text: 128 B a record + 32 B of per-record offsets, 4 B an op (the line's
    CIGAR and MC:Z:), the MD strings and the blobs, the names and the printed qualities up; the text down."""
    n_rec = ops = md = qual = 0
    op = re.compile(rb"[MIDSH]")
    for line in text.split(b"\n"):
        if not line:
            continue
        f = line.split(b"\t")
        n_rec += 1
        if f[5] != b"*":
            ops += len(op.findall(f[5]))
        if f[10] != b"*":
            qual += len(f[10])
        for t in f[11:]:
            if t.startswith(b"MD:Z:"):
                md += len(t) - 5
            elif t.startswith(b"MC:Z:"):
                ops += len(op.findall(t[5:]))
    names = n_rec * (name_bytes // max(n_reads, 1))
    up = {"records": 128 * n_rec, "record_offsets": 32 * n_rec, "ops": 4 * ops, "md_and_blobs": md + host_blob, "names": names, "qualities": qual}
    return {"records": n_rec, "up": up, "up_total": sum(up.values()), "down_text": len(text)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", default=None, help="load this libbm2.so instead of the tree's")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default="off,on")
    ap.add_argument("--pairs", type=int, default=500000)
    ap.add_argument("--genome-mbp", type=int, default=int(os.environ.get("BM2_BENCH_GENOME_MBP", 3100)))
    ap.add_argument("--workdir", default=os.environ.get("BM2_BENCH_WORKDIR", "/tmp/bm2_bench"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--bit", default="text", choices=("text", "decide", "both", "rescue", "rescue+decide", "all", "plan", "plan+rescue", "plan+rescue+decide+text", "pestat", "pestat+plan", "cgplan", "all+cgplan", "semark", "semark+cgplan", "cgprep", "all+cgplan+cgprep", "semark+cgplan+cgprep"))
    ap.add_argument("--single-end", action="store_true")
    a = ap.parse_args()
    if "semark" in a.bit:
        a.single_end = True
    res = {}
    if a.parent_lib:                                             # the baseline first, in a process of its own
        tmp = a.out + ".parent.json"
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--out", tmp, "--lib", a.parent_lib, "--variants", "off", "--pairs", str(a.pairs),
                               "--genome-mbp", str(a.genome_mbp), "--workdir", a.workdir, "--calls", str(a.calls), "--threads", str(a.threads)] + (["--single-end"] if a.single_end else []))
        res["parent"] = json.load(open(tmp))
        os.remove(tmp)
    import bench
    import bm2
    if a.lib:
        bm2.LIB_PATH = a.lib
    os.makedirs(a.workdir, exist_ok=True)
    prefix, contigs = bench.prepare_genome(a.workdir, a.genome_mbp, bench.SEED)
    fa, fb = os.path.join(a.workdir, "ab_1.fq"), os.path.join(a.workdir, "ab_2.fq")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_chunk.py"), prefix + ".contigs.npz", "901", str(a.pairs), "150", fa, fb, "s_"])
    t1, t2 = open(fa, "rb").read(), open(fb, "rb").read()
    os.remove(fa); os.remove(fb)
    ctx = bm2.Context(0, prefix)
    opt = bm2.default_opt()
    ch = bm2.FastqChunk(t1 + t2, None, 16) if a.single_end else bm2.FastqChunk(t1, t2, 16)
    paired = not a.single_end
    ctx.batch_upload_chunk(ch); ctx.batch_run(opt); ctx.batch_finish(opt)
    aln, aln_off = ctx.batch_download_alnregs()
    variants = a.variants.split(",")
    on = set({"both": "text+decide", "all": "text+decide+rescue", "all+cgplan": "text+decide+rescue+plan+pestat+cgplan", "all+cgplan+cgprep": "text+decide+rescue+plan+pestat+cgplan+cgprep"}.get(a.bit, a.bit).split("+"))
    bits = (getattr(bm2, "SAM_F_DEVICE_TEXT", 0) if "text" in on else 0) | (getattr(bm2, "SAM_F_DEVICE_DECIDE", 0) if "decide" in on else 0) | \
           (getattr(bm2, "SAM_F_DEVICE_RESCUE", 0) if "rescue" in on else 0) | (getattr(bm2, "SAM_F_DEVICE_PLAN", 0) if "plan" in on else 0) | (getattr(bm2, "SAM_F_DEVICE_PESTAT", 0) if "pestat" in on else 0) | \
           (getattr(bm2, "SAM_F_DEVICE_CGPLAN", 0) if "cgplan" in on else 0) | (getattr(bm2, "SAM_F_DEVICE_SEMARK", 0) if "semark" in on else 0) | \
           (getattr(bm2, "SAM_F_DEVICE_CGPREP", 0) if "cgprep" in on else 0)
    flag = {"off": 0, "on": bits}
    bufs = {v: bm2.Pinned(int(3 * (int(ch.f.n_bases) + 200 * ch.n_reads))) for v in variants}     # page-locked, as the pipeline's text buffers are
    so = {v: bm2.default_sam_opt(n_threads=a.threads, flag=flag[v]) for v in variants}
    if a.once:
        txt = ctx.sam(ch, opt, so["on"], aln, aln_off, 0, paired, out=bufs["on"].a)
        print("[ab] one bit-on call: %d bytes, counters %s" % (len(txt), bm2.sam_text_stats()), file=sys.stderr)
        return
    wall = {v: [] for v in variants}
    cpu = {v: [] for v in variants}
    ph = {v: [] for v in variants}
    counters, first, decided, rescued, planned_dev, model_dev, cgplan_dev, semark_dev, cgprep_dev = None, None, None, None, None, None, None, None, None
    os.environ["BM2_TAIL_PROF"] = "1"
    for rep in range(2 + a.calls):
        texts = {}
        for v in variants:
            c0 = cpu_s(); t0 = time.perf_counter()
            with Stderr() as err:
                txt = ctx.sam(ch, opt, so[v], aln, aln_off, 0, paired, out=bufs[v].a)
            dt, dc = time.perf_counter() - t0, cpu_s() - c0
            texts[v] = txt
            if v == "on" and "text" in on:
                counters = bm2.sam_text_stats()
            if v == "on" and "decide" in on:
                decided = bm2.sam_decide_stats()
            if v == "on" and "rescue" in on:
                rescued = bm2.sam_rescue_apply_stats() + bm2.sam_rescue_stats()
            if v == "on" and "plan" in on:
                planned_dev = bm2.sam_rescue_plan_stats() + bm2.sam_rescue_stats()
            if v == "on" and "pestat" in on:
                model_dev = bm2.sam_pestat_stats()
            if v == "on" and "cgplan" in on:
                cgplan_dev = bm2.sam_cigar_plan_stats() + bm2.sam_cigar_stats()
            if v == "on" and "semark" in on:
                semark_dev = bm2.sam_se_mark_stats() + bm2.sam_cigar_stats()
            if v == "on" and "cgprep" in on:
                cgprep_dev = bm2.sam_cigar_prep_stats()
            if rep >= 2:
                wall[v].append(dt * 1e3); cpu[v].append(dc); ph[v].append(phases(err.text))
        if len(variants) == 2:
            assert len(texts["off"]) == len(texts["on"]) and (texts["off"] == texts["on"]).all(), "call %d: the two texts differ" % rep
        if first is None:
            first = texts[variants[0]].tobytes()
        print("[ab] call %d: %s" % (rep, {v: "%.1f ms" % (wall[v][-1] if wall[v] else 0.0) for v in variants}), file=sys.stderr, flush=True)
    mine = {"reads": ch.n_reads, "single_end": bool(a.single_end), "text_bytes": len(first), "threads": a.threads, "lib": a.lib or "tree", "bit": a.bit, "variants": {}}
    for v in variants:
        keys = sorted(set(k for p in ph[v] for k in p))
        mine["variants"][v] = {"wall_ms": spread(wall[v]), "cpu_s": spread(cpu[v]),
                               "phases_ms_median": {k: float(np.median([p.get(k, 0.0) for p in ph[v]])) for k in keys}}
    if counters is not None:
        mine["text_stats"] = dict(zip(("records", "device_bytes", "host_bytes"), counters))
        name_bytes = sum(len(n) for n in ch.names())
        mine["pcie"] = pcie_ledger(first, ch.n_reads, name_bytes, counters[2])
    if decided is not None:                                      # (decide.hip: 56 B a hit and 8 B a list up, the tables aside; 32 B a hit and 32 B a pair down)
        pairs, hits, heavy = decided
        mine["decide_stats"] = {"pairs": pairs, "hits": hits, "pairs_heavy": heavy}
        mine["decide_pcie"] = {"up": 56 * hits + 8 * (2 * pairs + 1), "down": 32 * hits + 32 * pairs,
                               "up_per_pair": (56 * hits + 16 * pairs) / max(pairs, 1), "down_per_pair": (32 * hits + 32 * pairs) / max(pairs, 1)}
    if rescued is not None:                                      # (rescue.hip: 96 B a hit, 64 + 28 B a task, 8 B a list, 12 B a pair up; 96 B a hit, 8 B a list, 8 B a pair down)
        pairs, tasks, added, redone, planned, used, missed = rescued
        n_hits = int(aln_off[-1])
        mine["rescue_stats"] = {"pairs": pairs, "tasks": tasks, "hits_added": added, "pairs_redone": redone, "planned": planned, "missed_in_redo": missed}
        mine["rescue_pcie"] = {"up": 96 * n_hits + 92 * tasks + 8 * (2 * pairs + 1) + 8 * (pairs + 1) + 8 * pairs + 4 * pairs,
                               "down_at_most": 96 * (n_hits + added) + 8 * (2 * pairs + 1) + 8 * pairs}
    if planned_dev is not None:                                  # (plan.hip: 96 B a hit, 8 B a list offset, 4 B a read length up, 64 B a task and 8 B a pair down; the queries: the
        pairs, tasks, q_bytes, planned, used, missed = planned_dev      #  mates' run of codes -- at most the chunk's -- and 24 B a task up INSTEAD of the oriented queries)
        n_hits = int(aln_off[-1])
        mine["plan_stats"] = {"pairs": pairs, "tasks": tasks, "query_bytes": q_bytes, "planned": planned, "used": used, "missed": missed}
        mine["plan_pcie"] = {"plan_up": 96 * n_hits + 8 * (2 * pairs + 1) + 4 * 2 * pairs, "plan_down": 64 * tasks + 8 * (pairs + 1),
                             "queries_up_at_most": int(ch.f.n_bases) + 24 * tasks, "queries_up_without_the_bit": q_bytes}
    if model_dev is not None:                                    # (pestat.hip: 96 B a hit and 8 B a list offset up, 16 B a bin of one orientation down)
        pairs, counted, up, shared = model_dev
        mine["pestat_stats"] = {"pairs": pairs, "counted": counted, "hit_bytes_up": up, "hit_bytes_shared": shared}
        mine["pestat_pcie"] = {"up": up + 8 * (2 * pairs + 1), "down": 16 * (so["on"].max_ins + 1), "plan_up_saved": shared + (8 * (2 * pairs + 1) if shared else 0)}
    if cgplan_dev is not None:                                   # (cgplan.hip: 16 B a hit, 8 B a list offset and 32 B a pair up; 4 B a selected hit down)
        lists, hits, selected, heavy, planned, used, missed = cgplan_dev
        mine["cgplan_stats"] = {"lists": lists, "hits": hits, "selected": selected, "lists_heavy": heavy, "planned": planned, "used": used, "missed": missed}
        mine["cgplan_pcie"] = {"up": 16 * hits + 8 * (lists + 1) + 32 * (lists // 2), "down": 4 * selected + 12}
        if "semark" in on:                                       # (the marked lists and their offsets lie on the device already: 12 B a heavy list go up)
            mine["cgplan_pcie"]["up"] = 12 * heavy
    if semark_dev is not None:                                   # (semark.hip: 20 B a hit and 8 B a list offset up; 32 B a hit down; with cgplan the 16 B a hit stay on the device)
        lists, hits, heavy, planned, used, missed = semark_dev
        mine["semark_stats"] = {"lists": lists, "hits": hits, "lists_heavy": heavy, "planned": planned, "used": used, "missed": missed}
        mine["semark_pcie"] = {"up": 20 * hits + 8 * (lists + 1), "down": 32 * hits + 8, "cgplan_up_saved": 16 * hits if "cgplan" in on else 0}
    if cgprep_dev is not None:                                   # (cgprep.hip: 40 B a task and 12 B a read up INSTEAD of 76 B a task; 72 B of totals and error words down)
        tasks, shape, up, fallbacks = cgprep_dev
        mine["cgprep_stats"] = {"tasks": tasks, "ring": shape[0], "row": shape[1], "global": shape[2], "flat": shape[3], "bytes_up": up, "host_fallbacks": fallbacks}
        mine["cgprep_pcie"] = {"up": up, "up_without_the_bit": 76 * tasks, "down": 72}
    res.update(mine) if not a.parent_lib else res.update({"new": mine})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res if not a.parent_lib else {"parent": {k: res["parent"]["variants"]["off"][k] for k in ("wall_ms", "cpu_s")},
                                                   "new": {v: {k: mine["variants"][v][k] for k in ("wall_ms", "cpu_s")} for v in variants}}))


if __name__ == "__main__":
    main()
