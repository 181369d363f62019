"""What the depth bins cost on the device and through `coverm-amd depth --bin-size`, beside the run kernels of the same chunk and beside the
only way to the same numbers without them: Session.depth_runs() plus binning in numpy on the host.

    python tools/depth_bins_probe.py [--reads 50000000] [--contigs 5000] [--bp 1000000000]
                                     [--many-contigs 200000] [--many-bp 260000000] [--many-reads 2400000] [--out profiles/depth_bins_device.json]

The two synthetic sorted samples of tools/depth_runs_probe.py.  Each sample runs in a process of its own under a time limit (a sample that
fails or runs out of time ends the probe: nothing else is started).  In one session, for B = 100, 1 000 and 10 000, Session.depth_bins and
Session.depth_runs alternate (--reps times each): per chunk the HIP-event time of the bin kernels (COV_K_DEPTH_BINS), of the arena pass and
of the run kernels (COV_K_DEPTH_RUNS), the bins emitted and the bin kernels' algorithmic bytes over their time; per
call its wall time and the bytes fetched.  The host route expands the fetched runs of a chunk and reduces them with numpy's reduceat; its
bins are compared with the device's.  The sample written as a BAM file goes through `coverm-amd depth -o /dev/null -t 16` with and without
--bin-size 1000, whole process, COVERM_CLI_TIMING=1."""
import argparse
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BIN_SIZES = (100, 1000, 10000)


def algorithmic_bytes(arena_bases, n_bins, n_targets):
    """Bin kernels: the arena read once (16 B per word), the start mask and its rank (one bit and 1/32 word per arena word: written by the
    marks and the rank scan, read by the reduction), the bins initialised and written (24 B each, twice), the targets' offsets (woff and
    bin_off read)."""
    words = arena_bases // 4
    return 4 * arena_bases + 2 * (words // 8) + 2 * (words // 32) * 4 + 2 * 24 * n_bins + 8 * n_targets


def host_bins(lens, run_off, start, depth, sizes):
    """The bins of targets with lengths `lens` from their runs: the runs expanded to one depth per base, then reduceat per bin size."""
    from coverm_amd import native
    lens = np.asarray(lens, np.int64)
    ro = run_off.astype(np.int64)
    owner = np.repeat(np.arange(len(lens)), np.diff(ro))
    nxt = np.append(start[1:], 0).astype(np.int64)
    last = np.zeros(len(start), bool)
    last[ro[1:][ro[1:] > ro[:-1]] - 1] = True
    end = np.where(last, lens[owner], nxt)
    flat = np.repeat(depth, end - start.astype(np.int64))
    tstart = np.concatenate([[0], np.cumsum(lens)])[:-1]
    out = {}
    for B in sizes:
        nb = (lens + B - 1) // B
        boff = np.concatenate([[0], np.cumsum(nb)])
        idx = np.repeat(tstart, nb) + (np.arange(boff[-1]) - np.repeat(boff[:-1], nb)) * B
        bins = np.zeros(int(boff[-1]), native.DEPTH_BIN_DTYPE)
        if len(bins):
            bins["sum"] = np.add.reduceat(flat.astype(np.int64), idx)
            bins["min"] = np.minimum.reduceat(flat, idx)
            bins["max"] = np.maximum.reduceat(flat, idx)
            bins["covered"] = np.add.reduceat((flat > 0).astype(np.int64), idx)
        out[B] = (boff.astype(np.uint64), bins)
    return out


def one_sample(tag, n_contigs, bp, n_reads, seed, tmp, limit, reps, **ref_kw):
    from coverm_amd import bam as cbam
    from coverm_amd import synth
    from coverm_amd.engine import FilterConfig, Session
    from tests import binary
    t0 = time.perf_counter()
    ref = synth.make_reference(n_contigs, bp, seed=seed, **ref_kw)
    batch = synth.make_reads(ref, n_reads, seed=seed + 1)
    lens = np.asarray(ref.lengths, np.int64)
    res = dict(contigs=n_contigs, bases=int(lens.sum()), records=batch.n_records, generation_s=round(time.perf_counter() - t0, 3), bin_sizes={})
    print("[probe] %s: sample generated in %.1fs" % (tag, res["generation_s"]), flush=True)
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(ref.lengths)
        s.push(batch)
        s.finish()
        s.depth_runs(0, min(n_contigs, 64))      # warm-up: buffers of the first chunk, the kernels' code
        s.depth_bins(1000, 0, min(n_contigs, 64))
        device = {}
        for B in BIN_SIZES:
            per_rep = []
            for _ in range(reps):      # the two routes alternate in the one session
                cb, cr = [], []
                t0 = time.perf_counter()
                off, bins = s.depth_bins(B, chunks=cb)
                wall_b = time.perf_counter() - t0
                t0 = time.perf_counter()
                run_off, start, depth = s.depth_runs(chunks=cr)
                wall_r = time.perf_counter() - t0
                per_rep.append((sum(c["bins_ms"] for c in cb), wall_b, sum(c["runs_ms"] for c in cr), wall_r, cb, cr))
                n_runs = len(start)
                del run_off, start, depth
            device[B] = (off, bins)
            best = min(per_rep, key=lambda r: r[0])
            cb, cr = best[4], best[5]
            res["bin_sizes"][str(B)] = dict(
                bins=int(len(bins)), bins_bytes_fetched=int(bins.nbytes + off.nbytes), runs=int(n_runs), runs_bytes_fetched=int(8 * n_runs + off.nbytes),
                bin_kernels_ms_total=[round(r[0], 4) for r in per_rep], depth_bins_wall_s=[round(r[1], 4) for r in per_rep],
                run_kernels_ms_total=[round(r[2], 4) for r in per_rep], depth_runs_wall_s=[round(r[3], 4) for r in per_rep],
                chunks=[dict(targets=c["tid_next"] - c["tid_lo"], arena_bases=c["arena_bases"], bins=c["n_bins"], arena_pass_ms=round(c["arena_ms"], 4),
                             bin_kernels_ms=round(c["bins_ms"], 4), run_kernels_ms_same_chunk=round(r["runs_ms"], 4),
                             bin_kernels_algorithmic_bytes=algorithmic_bytes(c["arena_bases"], c["n_bins"], c["tid_next"] - c["tid_lo"]),
                             bin_kernels_tb_per_s=round(algorithmic_bytes(c["arena_bases"], c["n_bins"], c["tid_next"] - c["tid_lo"]) / (c["bins_ms"] * 1e-3) / 1e12, 4))
                        for c, r in zip(cb, cr)])
            print("[probe] %s B=%d: %d bins; bin kernels %s ms, run kernels %s ms; depth_bins %s s, depth_runs %s s" %
                  (tag, B, len(bins), res["bin_sizes"][str(B)]["bin_kernels_ms_total"], res["bin_sizes"][str(B)]["run_kernels_ms_total"],
                   res["bin_sizes"][str(B)]["depth_bins_wall_s"], res["bin_sizes"][str(B)]["depth_runs_wall_s"]), flush=True)
        # the host route, a chunk of the planner at a time: fetch the runs, expand, reduceat
        t_fetch = t_numpy = 0.0
        equal = True
        at = {B: 0 for B in BIN_SIZES}
        lo = 0
        for c in cr:
            t0 = time.perf_counter()
            run_off, start, depth = s.depth_runs(c["tid_lo"], c["tid_next"])
            t_fetch += time.perf_counter() - t0
            t0 = time.perf_counter()
            hb = host_bins(lens[c["tid_lo"]:c["tid_next"]], run_off, start, depth, BIN_SIZES)
            t_numpy += time.perf_counter() - t0
            for B in BIN_SIZES:
                off, bins = device[B]
                n = len(hb[B][1])
                lo_b = int(off[c["tid_lo"]])
                equal = equal and bins[lo_b:lo_b + n].tobytes() == hb[B][1].tobytes() and bool((off[c["tid_lo"]:c["tid_next"] + 1] - off[c["tid_lo"]] == hb[B][0]).all())
                at[B] += n
            del run_off, start, depth, hb
            lo = c["tid_next"]
        equal = equal and lo == n_contigs and all(at[B] == len(device[B][1]) for B in BIN_SIZES)
        res["host_route"] = dict(depth_runs_fetch_wall_s=round(t_fetch, 4), numpy_expand_and_reduceat_three_sizes_wall_s=round(t_numpy, 4), bins_equal=bool(equal))
        print("[probe] %s: host route: runs fetched in %.3fs, numpy %.3fs, equal %s" % (tag, t_fetch, t_numpy, equal), flush=True)
    del device
    path = os.path.join(tmp, tag + ".bam")
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=1, threads=16)
    res["bam_bytes"] = os.path.getsize(path)
    for name, extra, word in (("cli_depth", [], "depth runs"), ("cli_depth_bin_size_1000", ["--bin-size", "1000"], "depth bins"), ("cli_depth_again", [], "depth runs"),
                              ("cli_depth_bin_size_1000_again", ["--bin-size", "1000"], "depth bins")):
        t0 = time.perf_counter()
        r = subprocess.run([binary.BIN, "depth", "-b", path, "-o", "/dev/null", "-t", "16"] + extra, capture_output=True, text=True, timeout=limit,
                           env=dict(os.environ, COVERM_CLI_TIMING="1"))
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("the binary failed: %s" % r.stderr[-2000:])
        res[name] = dict(wall_s=round(dt, 3), timing=[l for l in r.stderr.splitlines() if word in l and "sample" in l][:1])
        print("[probe] %s: coverm-amd depth %s: %.3fs" % (tag, " ".join(extra), dt), flush=True)
    os.remove(path)
    return res


SAMPLES = {"config2": lambda a: dict(n_contigs=a.contigs, bp=a.bp, n_reads=a.reads, seed=1),
           "many_contigs": lambda a: dict(n_contigs=a.many_contigs, bp=a.many_bp, n_reads=a.many_reads, seed=21, min_len=1000, max_len=40_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--bp", type=int, default=1_000_000_000)
    ap.add_argument("--many-contigs", type=int, default=200_000)
    ap.add_argument("--many-bp", type=int, default=260_000_000)
    ap.add_argument("--many-reads", type=int, default=2_400_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one run of the binary, seconds")
    ap.add_argument("--sample-limit", type=int, default=900, help="time limit of one sample's whole process (generation, device loops, numpy, four runs of the binary), seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_bins_device.json"))
    ap.add_argument("--sample", choices=sorted(SAMPLES), help="(internal) run this sample in this process and write its result to --out")
    a = ap.parse_args()
    if a.sample:
        with tempfile.TemporaryDirectory() as tmp:
            res = one_sample(a.sample, tmp=tmp, limit=a.limit, reps=a.reps, **SAMPLES[a.sample](a))
        with open(a.out, "w") as fh:
            json.dump(res, fh)
        return
    out = {"what": "depth bins: COV_K_DEPTH_BINS, the arena pass and COV_K_DEPTH_RUNS per chunk in one session, alternating; bins emitted; the host route "
                   "(Session.depth_runs + numpy); wall time of `coverm-amd depth` with and without --bin-size 1000 (tools/depth_bins_probe.py)",
           "peak_hbm_tb_per_s": 8.0}
    with tempfile.TemporaryDirectory() as tmp:
        for tag in ("config2", "many_contigs"):
            part = os.path.join(tmp, tag + ".json")
            argv = [sys.executable, os.path.abspath(__file__), "--sample", tag, "--out", part, "--limit", str(a.limit), "--reps", str(a.reps)]
            for k in ("reads", "contigs", "bp", "many_contigs", "many_bp", "many_reads"):
                argv += ["--" + k.replace("_", "-"), str(getattr(a, k))]
            # a fresh process per sample, in a process group of its own: when its limit runs out the whole group is killed, a run of the
            # binary under it included, so that nothing is left with the device open; a failure ends the probe
            p = subprocess.Popen(argv, start_new_session=True)
            try:
                rc = p.wait(timeout=a.sample_limit)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                raise SystemExit("sample %s ran out of its %d s: its process group was killed, nothing else is started" % (tag, a.sample_limit))
            if rc != 0:
                raise SystemExit("sample %s failed with status %d: nothing else is started" % (tag, rc))
            with open(part) as fh:
                out[tag] = json.load(fh)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "bin_sizes"} if isinstance(v, dict) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
