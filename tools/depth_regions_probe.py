"""What the depth regions cost on the device and through `coverm-amd depth --regions`, beside the two things nearest to them: the depth bins
of the same session (the yardstick for regions that tile the contigs) and cov_interval_stats_compute over the same intervals (--gff's
reduction: why a new kernel).

    python tools/depth_regions_probe.py [--reads 50000000] [--contigs 5000] [--bp 1000000000] [--runs 5] [--out profiles/depth_regions_device.json]

One config-2-sized synthetic sorted sample (coverm_amd/synth.py) and four region sets over it:
    tiles_1000     windows of 1 000 bases tiling every contig; beside it COV_K_DEPTH_BINS of depth_bins(1000), whose bytes must be equal
    random_200k    200 000 random regions of 100 .. 300 bases
    whole_contigs  one region per contig; beside it the wall time of cov_interval_stats_compute over the same intervals (no histograms)
    genes_1m       1 000 000 gene-like regions of about 1 kb
Each of --runs runs is a process of its own under a time limit (a run that fails or runs out of time ends the probe: nothing else is
started); per set it records the region kernels' ms (COV_K_DEPTH_REGIONS) and the arena pass summed over the chunks, the pieces, the wall
time of Session.depth_regions and the bytes fetched.  The recorded figure is the median over the runs.  The sample written as a BAM file
then goes through `coverm-amd depth --regions <set>.bed -o /dev/null -t 16`, --runs times per set, whole process."""
import argparse
import ctypes as C
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
sys.path.insert(0, ROOT)

SETS = ("tiles_1000", "random_200k", "whole_contigs", "genes_1m")


def region_set(name, lens, seed=7):
    """A native.DEPTH_REGION_DTYPE array over contigs of lengths `lens`, deterministic."""
    from coverm_amd import native
    lens = np.asarray(lens, np.int64)
    rng = np.random.default_rng(seed)
    if name == "tiles_1000":
        nb = (lens + 999) // 1000
        tid = np.repeat(np.arange(len(lens)), nb)
        start = (np.arange(int(nb.sum())) - np.repeat(np.cumsum(nb) - nb, nb)) * 1000
        end = np.minimum(start + 1000, lens[tid])
    elif name == "whole_contigs":
        tid, start, end = np.arange(len(lens)), np.zeros(len(lens), np.int64), lens.copy()
    else:
        n, lo, hi = (200_000, 100, 301) if name == "random_200k" else (1_000_000, 600, 1401)
        tid = np.searchsorted(np.cumsum(lens) / lens.sum(), rng.random(n), side="right").clip(0, len(lens) - 1)      # by length
        size = np.minimum(rng.integers(lo, hi, n), lens[tid])
        start = (rng.random(n) * (lens[tid] - size + 1)).astype(np.int64)
        end = start + size
    out = np.zeros(len(tid), native.DEPTH_REGION_DTYPE)
    out["tid"], out["start"], out["end"] = tid, start, end
    assert (out["start"] < out["end"]).all() and (out["end"] <= lens[out["tid"]]).all()
    return out


def algorithmic_bytes(regions):
    """Region kernels: 4 B per base of every region read from the arena, 24 B per region written."""
    return int(4 * (regions["end"].astype(np.int64) - regions["start"]).sum() + 24 * len(regions))


def one_run(a):
    from coverm_amd import native, synth
    from coverm_amd.engine import FilterConfig, Session
    ref = synth.make_reference(a.contigs, a.bp, seed=1)
    batch = synth.make_reads(ref, a.reads, seed=2)
    lens = np.asarray(ref.lengths, np.int64)
    res = dict(contigs=a.contigs, bases=int(lens.sum()), records=batch.n_records, sets={})
    L = native.lib()
    L.cov_interval_stats_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(ref.lengths)
        s.push(batch)
        s.finish()
        s.set_depth_regions(region_set("whole_contigs", lens[:8]))      # warm-up: buffers of a first chunk, the kernels' code
        s.depth_regions()
        s.depth_bins(1000, 0, min(a.contigs, 8))
        for name in SETS:
            regs = region_set(name, lens)
            s.set_depth_regions(regs)
            chunks = []
            t0 = time.perf_counter()
            out = s.depth_regions(chunks=chunks)
            wall = time.perf_counter() - t0
            ms = sum(c["regions_ms"] for c in chunks)
            r = dict(regions=int(len(regs)), pieces=int(sum(c["n_pieces"] for c in chunks)), chunks=len(chunks), region_kernels_ms=round(ms, 4),
                     arena_pass_ms=round(sum(c["arena_ms"] for c in chunks), 4), depth_regions_wall_s=round(wall, 4), bytes_fetched=int(out.nbytes + 8 * len(out)),
                     algorithmic_bytes=algorithmic_bytes(regs), algorithmic_tb_per_s=round(algorithmic_bytes(regs) / (ms * 1e-3) / 1e12, 4))
            if name == "tiles_1000":
                cb = []
                t0 = time.perf_counter()
                _, bins = s.depth_bins(1000, chunks=cb)
                r.update(depth_bins_1000_wall_s=round(time.perf_counter() - t0, 4), bin_kernels_ms=round(sum(c["bins_ms"] for c in cb), 4),
                         bins_arena_pass_ms=round(sum(c["arena_ms"] for c in cb), 4), bytes_equal_to_depth_bins=bool(bins.tobytes() == out.tobytes()))
            if name == "whole_contigs":
                iv = np.zeros(len(regs), native.INTERVAL_DTYPE)
                iv["tid"], iv["start"], iv["end"] = regs["tid"], regs["start"], regs["end"]
                st = np.zeros(len(regs), np.dtype([("win_sum_d", "<u8"), ("win_sum_d2", "<u8"), ("win_covered", "<u8"), ("full_covered", "<u8"), ("win_min_d", "<u4"),
                                                   ("win_max_d", "<u4"), ("hist_len", "<u4"), ("pad", "<u4"), ("hist_off", "<u8")]))
                tot = C.c_uint64(0)
                walls = []
                for _ in range(2):      # the second call finds its buffers
                    t0 = time.perf_counter()
                    s._check(L.cov_interval_stats_compute(s._h, iv.ctypes.data, len(iv), 0, 0, st.ctypes.data, C.byref(tot)))
                    walls.append(round(time.perf_counter() - t0, 4))
                r.update(interval_stats_compute_wall_s=walls, interval_stats_equal=bool((st["win_sum_d"] == out["sum"]).all() and (st["win_max_d"] == out["max"]).all()
                                                                                         and (st["full_covered"] == out["covered"]).all()))
            res["sets"][name] = r
            print("[probe] %s: %s" % (name, json.dumps(r)), flush=True)
    return res, ref, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--bp", type=int, default=1_000_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one run of the binary, seconds")
    ap.add_argument("--run-limit", type=int, default=300, help="time limit of one run's whole process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_regions_device.json"))
    ap.add_argument("--run", help="(internal) one run in this process: its result goes to this file; with --bam-dir the sample and the BED files are written there")
    ap.add_argument("--bam-dir")
    a = ap.parse_args()
    if a.run:
        res, ref, batch = one_run(a)
        if a.bam_dir:
            from coverm_amd import bam as cbam
            cbam.write_bam(os.path.join(a.bam_dir, "sample.bam"), ref.names, ref.lengths, batch, with_seq=1, threads=16)
            for name in SETS:
                regs = region_set(name, ref.lengths)
                names = np.asarray(ref.names, dtype=object)[regs["tid"]]
                with open(os.path.join(a.bam_dir, name + ".bed"), "w") as fh:
                    fh.write("".join("%s\t%d\t%d\n" % t for t in zip(names, regs["start"].tolist(), regs["end"].tolist())))
        with open(a.run, "w") as fh:
            json.dump(res, fh)
        return
    from tests import binary
    out = {"what": "depth regions: COV_K_DEPTH_REGIONS and the arena pass summed over the chunks of one sample, per region set, median of %d one-process runs; "
                   "COV_K_DEPTH_BINS of depth_bins(1000) beside the tiling set, cov_interval_stats_compute beside the whole contigs; wall time of "
                   "`coverm-amd depth --regions` (tools/depth_regions_probe.py)" % a.runs, "peak_hbm_tb_per_s": 8.0, "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(a.runs):
            part = os.path.join(tmp, "run%d.json" % i)
            argv = [sys.executable, os.path.abspath(__file__), "--run", part, "--reads", str(a.reads), "--contigs", str(a.contigs), "--bp", str(a.bp)]
            if i == a.runs - 1:
                argv += ["--bam-dir", tmp]
            # a fresh process per run, in a process group of its own: when its limit runs out the whole group is killed, so that nothing is
            # left with the device open; a failure ends the probe
            p = subprocess.Popen(argv, start_new_session=True)
            try:
                rc = p.wait(timeout=a.run_limit)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                raise SystemExit("run %d ran out of its %d s: its process group was killed, nothing else is started" % (i, a.run_limit))
            if rc != 0:
                raise SystemExit("run %d failed with status %d: nothing else is started" % (i, rc))
            with open(part) as fh:
                out["runs"].append(json.load(fh))
        med = {}
        for name in SETS:
            first = out["runs"][0]["sets"][name]
            m = {k: first[k] for k in ("regions", "pieces", "chunks", "bytes_fetched", "algorithmic_bytes")}
            for k, v in first.items():
                if isinstance(v, float):
                    m[k] = round(statistics.median(r["sets"][name][k] for r in out["runs"]), 4)
                elif isinstance(v, bool):
                    m[k] = all(r["sets"][name][k] for r in out["runs"])
            if "interval_stats_compute_wall_s" in first:
                m["interval_stats_compute_second_call_wall_s"] = round(statistics.median(r["sets"][name]["interval_stats_compute_wall_s"][1] for r in out["runs"]), 4)
            med[name] = m
        out["median"] = med
        out["bam_bytes"] = os.path.getsize(os.path.join(tmp, "sample.bam"))
        cli = {}
        for name in SETS + ("bin_size_1000",):
            extra = ["--bin-size", "1000"] if name == "bin_size_1000" else ["--regions", os.path.join(tmp, name + ".bed")]
            walls, lines = [], []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                r = subprocess.run([binary.BIN, "depth", "-b", os.path.join(tmp, "sample.bam"), "-o", "/dev/null", "-t", "16"] + extra, capture_output=True, text=True,
                                   timeout=a.limit, env=dict(os.environ, COVERM_CLI_TIMING="1"))
                walls.append(round(time.perf_counter() - t0, 3))
                if r.returncode != 0:
                    raise SystemExit("the binary failed: %s" % r.stderr[-2000:])
                lines = [l for l in r.stderr.splitlines() if ("depth regions" in l or "depth bins" in l) and "sample" in l][:1]
            cli[name] = dict(wall_s=walls, median_wall_s=round(statistics.median(walls), 3), timing_of_the_last_run=lines)
            print("[probe] coverm-amd depth %s: %s" % (name, walls), flush=True)
        out["cli"] = cli
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"median": out["median"], "cli": {k: v["median_wall_s"] for k, v in cli.items()}}))


if __name__ == "__main__":
    main()
