"""What the depth classes cost on the device and through `coverm-amd depth --quantize / --thresholds`, beside the paths they were built on.

    python tools/depth_classes_probe.py [--reads 50000000] [--contigs 5000] [--bp 1000000000] [--runs 5] [--out profiles/depth_classes_device.json]
                                        [--parent-tree DIR]

One config-2-sized synthetic sorted sample (coverm_amd/synth.py), as the other depth probes use.  Each of --runs runs is a process of its own
under a time limit (a run that fails or runs out of time ends the probe: nothing else is started) and records, alternating inside one session:
    runs          COV_K_DEPTH_RUNS summed over the chunks of Session.depth_runs and of Session.depth_class_runs((0, 1, 5, 150)), the runs
                  emitted, the bytes fetched and the wall time of the call
    thresholds    COV_K_DEPTH_REGIONS summed over the chunks for the gene-like regions and the whole contigs of tools/depth_regions_probe.py
                  with K = 0 (the plain kernel), 4 and 16 thresholds; for the whole contigs the arena bytes per second the kernel achieved
The recorded figure is the median over the runs.  The sample written as a BAM file then goes through the binary, whole process: the plain
track, `--quantize 0:1:5:150:`, and `--regions genes_1m.bed` without and with `--thresholds 1,10,30,100`.
--parent-tree DIR: a build of the parent commit (its coverm_amd package with libcovermhip.so and coverm-amd).  The unchanged paths (the plain
runs, the regions without thresholds) are then measured in processes that alternate between the two builds, and both series are recorded."""
import argparse
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUANTIZE = "0:1:5:150:"
CUTS = (0, 1, 5, 150)
THRESHOLDS = {0: (), 4: (1, 10, 30, 100), 16: tuple(range(1, 32, 2))}
REGION_SETS = ("genes_1m", "whole_contigs")


def sample(a):
    from coverm_amd import synth
    ref = synth.make_reference(a.contigs, a.bp, seed=1)
    return ref, synth.make_reads(ref, a.reads, seed=2)


def open_session(ref, batch):
    from coverm_amd.engine import FilterConfig, Session
    s = Session(0, FilterConfig(), 0)
    s.set_targets(ref.lengths)
    s.push(batch)
    s.finish()
    return s


def one_run(a):
    """The new paths beside the old ones, alternating in one session."""
    from tools.depth_regions_probe import region_set
    ref, batch = sample(a)
    lens = np.asarray(ref.lengths, np.int64)
    res = dict(contigs=a.contigs, bases=int(lens.sum()), records=batch.n_records, runs={"plain": [], "classes": []}, thresholds={})
    with open_session(ref, batch) as s:
        s.depth_runs(0, min(a.contigs, 8))      # warm-up: buffers of a first chunk, the kernels' code
        s.depth_class_runs(CUTS, 0, min(a.contigs, 8))
        for _ in range(a.reps):
            for kind in ("plain", "classes"):
                chunks = []
                t0 = time.perf_counter()
                off, start, _ = s.depth_runs(chunks=chunks) if kind == "plain" else s.depth_class_runs(CUTS, chunks=chunks)
                wall = time.perf_counter() - t0
                res["runs"][kind].append(dict(run_kernels_ms=round(sum(c["runs_ms"] for c in chunks), 4), arena_pass_ms=round(sum(c["arena_ms"] for c in chunks), 4),
                                              n_runs=int(len(start)), bytes_fetched=int(8 * len(start) + 8 * len(off)), wall_s=round(wall, 4), chunks=len(chunks)))
                del off, start
        print("[probe] runs: %s" % json.dumps(res["runs"]), flush=True)
        for name in REGION_SETS:
            regs = region_set(name, lens)
            s.set_depth_regions(regs)
            bases = int((regs["end"].astype(np.int64) - regs["start"]).sum())
            per = {str(k): [] for k in THRESHOLDS}
            for _ in range(a.reps):
                for k, thr in THRESHOLDS.items():
                    s.set_depth_thresholds(thr)
                    chunks = []
                    t0 = time.perf_counter()
                    if k:
                        s.depth_region_counts(chunks=chunks)
                    else:
                        s.depth_regions(chunks=chunks)
                    wall = time.perf_counter() - t0
                    ms = sum(c["regions_ms"] for c in chunks)
                    per[str(k)].append(dict(region_kernels_ms=round(ms, 4), wall_s=round(wall, 4), arena_tb_per_s=round(4 * bases / (ms * 1e-3) / 1e12, 4)))
            s.set_depth_thresholds(())
            res["thresholds"][name] = dict(regions=int(len(regs)), bases=bases, per_k=per)
            print("[probe] thresholds %s: %s" % (name, json.dumps(per)), flush=True)
    return res, ref, batch


def ab_run(a):
    """The unchanged paths of whichever build is first on sys.path."""
    from tools.depth_regions_probe import region_set
    ref, batch = sample(a)
    lens = np.asarray(ref.lengths, np.int64)
    res = {"plain_run_kernels_ms": [], "regions_genes_1m_ms": [], "regions_whole_contigs_ms": []}
    with open_session(ref, batch) as s:
        s.depth_runs(0, min(a.contigs, 8))
        sets = {name: region_set(name, lens) for name in REGION_SETS}
        for _ in range(a.reps):
            chunks = []
            s.depth_runs(chunks=chunks)
            res["plain_run_kernels_ms"].append(round(sum(c["runs_ms"] for c in chunks), 4))
            for name in REGION_SETS:
                s.set_depth_regions(sets[name])
                chunks = []
                s.depth_regions(chunks=chunks)
                res["regions_%s_ms" % name].append(round(sum(c["regions_ms"] for c in chunks), 4))
    return res


def child(argv, limit, what, env=None):
    """A fresh process in a process group of its own: when its limit runs out the whole group is killed, so that nothing is left with the
    device open; a failure ends the probe."""
    p = subprocess.Popen(argv, start_new_session=True, env=env)
    try:
        rc = p.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.wait()
        raise SystemExit("%s ran out of its %d s: its process group was killed, nothing else is started" % (what, limit))
    if rc != 0:
        raise SystemExit("%s failed with status %d: nothing else is started" % (what, rc))


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--bp", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="alternations inside one run")
    ap.add_argument("--ab-runs", type=int, help="processes per build of the comparison with --parent-tree (default: --runs)")
    ap.add_argument("--limit", type=int, default=120, help="time limit of one run of the binary, seconds")
    ap.add_argument("--run-limit", type=int, default=300, help="time limit of one run's whole process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_classes_device.json"))
    ap.add_argument("--parent-tree", help="a build of the parent commit: the directory that holds its coverm_amd package")
    ap.add_argument("--run", help="(internal) one run in this process: its result goes to this file; with --bam-dir the sample and the BED file are written there")
    ap.add_argument("--ab-run", help="(internal) the unchanged paths in this process, of the build in --tree")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--bam-dir")
    a = ap.parse_args()
    if a.ab_run:
        sys.path.insert(0, ROOT)      # tools.depth_regions_probe (no native code) ...
        sys.path.insert(0, os.path.abspath(a.tree))      # ... and in front of it the build under test, bound before anything else is imported
        import coverm_amd.native
        assert os.path.abspath(coverm_amd.native.LIB_PATH).startswith(os.path.abspath(a.tree) + os.sep), coverm_amd.native.LIB_PATH
        with open(a.ab_run, "w") as fh:
            json.dump(ab_run(a), fh)
        return
    sys.path.insert(0, ROOT)
    if a.run:
        res, ref, batch = one_run(a)
        if a.bam_dir:
            from coverm_amd import bam as cbam
            from tools.depth_regions_probe import region_set
            cbam.write_bam(os.path.join(a.bam_dir, "sample.bam"), ref.names, ref.lengths, batch, with_seq=1, threads=16)
            regs = region_set("genes_1m", ref.lengths)
            names = np.asarray(ref.names, dtype=object)[regs["tid"]]
            with open(os.path.join(a.bam_dir, "genes_1m.bed"), "w") as fh:
                fh.write("".join("%s\t%d\t%d\n" % t for t in zip(names, regs["start"].tolist(), regs["end"].tolist())))
        with open(a.run, "w") as fh:
            json.dump(res, fh)
        return
    from tests import binary
    size = ["--reads", str(a.reads), "--contigs", str(a.contigs), "--bp", str(a.bp), "--reps", str(a.reps)]
    out = {"what": "depth classes: COV_K_DEPTH_RUNS of the plain runs and of the class runs %s, alternating in one session; COV_K_DEPTH_REGIONS with 0, 4 and 16 "
                   "thresholds over gene-like regions and whole contigs; median of %d one-process runs of %d alternations each; wall time of the binary "
                   "(tools/depth_classes_probe.py)" % (QUANTIZE, a.runs, a.reps), "peak_hbm_tb_per_s": 8.0, "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(a.runs):
            part = os.path.join(tmp, "run%d.json" % i)
            argv = [sys.executable, os.path.abspath(__file__), "--run", part] + size
            if i == a.runs - 1:
                argv += ["--bam-dir", tmp]
            child(argv, a.run_limit, "run %d" % i)
            with open(part) as fh:
                out["runs"].append(json.load(fh))
        m = {"runs": {}, "thresholds": {}}
        for kind in ("plain", "classes"):
            rows = [x for r in out["runs"] for x in r["runs"][kind]]
            m["runs"][kind] = dict(run_kernels_ms=med([x["run_kernels_ms"] for x in rows]), arena_pass_ms=med([x["arena_pass_ms"] for x in rows]),
                                   wall_s=med([x["wall_s"] for x in rows]), n_runs=rows[0]["n_runs"], bytes_fetched=rows[0]["bytes_fetched"], chunks=rows[0]["chunks"])
        for name in REGION_SETS:
            first = out["runs"][0]["thresholds"][name]
            m["thresholds"][name] = dict(regions=first["regions"], bases=first["bases"])
            for k in THRESHOLDS:
                rows = [x for r in out["runs"] for x in r["thresholds"][name]["per_k"][str(k)]]
                m["thresholds"][name]["K=%d" % k] = dict(region_kernels_ms=med([x["region_kernels_ms"] for x in rows]), wall_s=med([x["wall_s"] for x in rows]),
                                                         arena_tb_per_s=med([x["arena_tb_per_s"] for x in rows]))
        out["median"] = m
        out["bam_bytes"] = os.path.getsize(os.path.join(tmp, "sample.bam"))
        bam, bed = os.path.join(tmp, "sample.bam"), os.path.join(tmp, "genes_1m.bed")
        modes = {"runs": [], "quantize": ["--quantize", QUANTIZE], "regions_genes_1m": ["--regions", bed],
                 "regions_genes_1m_thresholds_4": ["--regions", bed, "--thresholds", "1,10,30,100"]}
        bins = {"this_commit": binary.BIN}
        if a.parent_tree:
            bins["parent"] = os.path.join(os.path.abspath(a.parent_tree), "coverm_amd", "coverm-amd")
        cli = {b: {k: [] for k in modes if b == "this_commit" or "quantize" not in k and "thresholds" not in k} for b in bins}
        for _ in range(a.runs):      # the builds and the modes alternate
            for mode, extra in modes.items():
                for b, exe in bins.items():
                    if mode not in cli[b]:
                        continue
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "depth", "-b", bam, "-o", "/dev/null", "-t", "16"] + extra, capture_output=True, text=True, timeout=a.limit)
                    if r.returncode != 0:
                        raise SystemExit("the binary failed: %s" % r.stderr[-2000:])
                    cli[b][mode].append(round(time.perf_counter() - t0, 3))
        out["cli_wall_s"] = cli
        out["cli_median_wall_s"] = {b: {k: round(statistics.median(v), 3) for k, v in d.items()} for b, d in cli.items()}
        print("[probe] binary: %s" % json.dumps(out["cli_median_wall_s"]), flush=True)
        if a.parent_tree:
            ab = {"this_commit": [], "parent": []}
            for i in range(a.ab_runs or a.runs):
                for b, tree in (("this_commit", ROOT), ("parent", a.parent_tree)):
                    part = os.path.join(tmp, "ab_%s_%d.json" % (b, i))
                    child([sys.executable, os.path.abspath(__file__), "--ab-run", part, "--tree", tree] + size, a.run_limit, "A/B run %d of %s" % (i, b))
                    with open(part) as fh:
                        ab[b].append(json.load(fh))
            out["unchanged_paths_ab"] = {"what": "processes alternating between this commit's build and the parent's; per process %d measurements of each path, ms" % a.reps,
                                         "series": ab,
                                         "median": {b: {k: med([x for r in rs for x in r[k]]) for k in rs[0]} for b, rs in ab.items()},
                                         "min_max": {b: {k: [min(x for r in rs for x in r[k]), max(x for r in rs for x in r[k])] for k in rs[0]} for b, rs in ab.items()}}
            print("[probe] unchanged paths: %s" % json.dumps({k: out["unchanged_paths_ab"][k] for k in ("median", "min_max")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"median": out["median"], "cli": out["cli_median_wall_s"]}))


if __name__ == "__main__":
    main()
