"""What the depth runs cost on the device and through `coverm-amd depth`, beside the only way to the same output without them:
Session.depth(t) for every target plus a run-length encode in numpy.

    python tools/depth_runs_probe.py [--reads 50000000] [--contigs 5000] [--bp 1000000000]
                                     [--many-contigs 200000] [--many-bp 260000000] [--many-reads 2400000] [--out profiles/depth_runs_device.json]

Two synthetic sorted samples: one of bench.py's config-2 size (50 M reads over 5 000 contigs, 1 Gbp) and an assembly of 200 000 contigs.
For each: the records are pushed and finished once; Session.depth_runs gives, per chunk, the HIP-event time of the arena pass (zero fill +
pileup into the arena) and of the run kernels (COV_K_DEPTH_RUNS), the arena's entries and the runs emitted, and the wall time of the whole
call (compute + fetch + concatenation in Python); the per-target route's wall time is taken the same way and its runs are compared with the
device's; the sample written as a BAM file goes through one process of `coverm-amd depth -o /dev/null` (-t 16, COVERM_CLI_TIMING=1), whose
wall time and timing line are kept.  The run kernels' algorithmic bytes over their time give the achieved bandwidth
the file records beside the arena pass's own."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(arena_bases, n_runs, n_targets):
    """Run kernels: the arena read twice (count, emit: 4 B per entry each), the start mask and its rank (one bit and 1/32 word per word of
    four entries, read by both passes, written once), the runs written (8 B each), the targets' offsets (woff read, run_off written)."""
    words = arena_bases // 4
    return 2 * 4 * arena_bases + 2 * (words // 8) + 3 * (words // 32) * 4 + 8 * n_runs + 8 * n_targets


def rle_per_target(s, n_targets):
    starts, depths, off = [], [], [0]
    for t in range(n_targets):
        d = s.depth(t)
        if d.size:
            st = np.concatenate([[0], np.flatnonzero(np.diff(d)) + 1])
            starts.append(st.astype(np.uint32)); depths.append(d[st])
            off.append(off[-1] + len(st))
        else:
            off.append(off[-1])
    return np.asarray(off, np.uint64), np.concatenate(starts), np.concatenate(depths)


def one_sample(tag, n_contigs, bp, n_reads, seed, tmp, limit, **ref_kw):
    from coverm_amd import bam as cbam
    from coverm_amd import synth
    from coverm_amd.engine import FilterConfig, Session
    from tests import binary
    t0 = time.perf_counter()
    ref = synth.make_reference(n_contigs, bp, seed=seed, **ref_kw)
    batch = synth.make_reads(ref, n_reads, seed=seed + 1)
    res = dict(contigs=n_contigs, bases=int(np.sum(ref.lengths)), records=batch.n_records, generation_s=round(time.perf_counter() - t0, 3))
    print("[probe] %s: sample generated in %.1fs" % (tag, res["generation_s"]), flush=True)
    with Session(0, FilterConfig(), 0) as s:
        s.set_targets(ref.lengths)
        s.push(batch)
        s.finish()
        s.depth_runs(0, min(n_contigs, 64))      # warm-up: buffers of the first chunk, the kernels' code
        chunks = []
        t0 = time.perf_counter()
        run_off, start, depth = s.depth_runs(chunks=chunks)
        res["depth_runs_wall_s"] = round(time.perf_counter() - t0, 4)
        res["runs"] = int(len(start))
        res["chunks"] = [dict(targets=c["tid_next"] - c["tid_lo"], arena_bases=c["arena_bases"], runs=c["n_runs"], arena_pass_ms=round(c["arena_ms"], 4),
                              run_kernels_ms=round(c["runs_ms"], 4),
                              run_kernels_algorithmic_bytes=algorithmic_bytes(c["arena_bases"], c["n_runs"], c["tid_next"] - c["tid_lo"]),
                              run_kernels_tb_per_s=round(algorithmic_bytes(c["arena_bases"], c["n_runs"], c["tid_next"] - c["tid_lo"]) / (c["runs_ms"] * 1e-3) / 1e12, 4),
                              arena_write_tb_per_s=round(4 * c["arena_bases"] / (c["arena_ms"] * 1e-3) / 1e12, 4)) for c in chunks]
        res["arena_pass_ms_total"] = round(sum(c["arena_ms"] for c in chunks), 4)
        res["run_kernels_ms_total"] = round(sum(c["runs_ms"] for c in chunks), 4)
        print("[probe] %s: depth_runs %d runs in %d chunks, %.3fs wall (arena %.2f ms, run kernels %.2f ms)" %
              (tag, res["runs"], len(chunks), res["depth_runs_wall_s"], res["arena_pass_ms_total"], res["run_kernels_ms_total"]), flush=True)
        t0 = time.perf_counter()
        off2, start2, depth2 = rle_per_target(s, n_contigs)
        res["per_target_depth_plus_numpy_rle_wall_s"] = round(time.perf_counter() - t0, 4)
        res["routes_equal"] = bool((off2 == run_off).all() and (start2 == start).all() and (depth2 == depth).all())
        print("[probe] %s: Session.depth per target + numpy: %.3fs, equal %s" % (tag, res["per_target_depth_plus_numpy_rle_wall_s"], res["routes_equal"]), flush=True)
    del run_off, start, depth, off2, start2, depth2
    path = os.path.join(tmp, tag + ".bam")
    t0 = time.perf_counter()
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=1, threads=16)
    res["bam_bytes"] = os.path.getsize(path)
    res["bam_write_s"] = round(time.perf_counter() - t0, 3)
    for name, extra in (("cli_depth", []), ("cli_depth_no_zeros", ["--no-zeros"])):
        t0 = time.perf_counter()
        r = subprocess.run([binary.BIN, "depth", "-b", path, "-o", "/dev/null", "-t", "16"] + extra, capture_output=True, text=True, timeout=limit,
                           env=dict(os.environ, COVERM_CLI_TIMING="1"))
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit("the binary failed: %s" % r.stderr[-2000:])
        res[name] = dict(wall_s=round(dt, 3), timing=[l for l in r.stderr.splitlines() if "depth runs" in l and "sample" in l][:1])
        print("[probe] %s: coverm-amd depth %s: %.3fs" % (tag, " ".join(extra), dt), flush=True)
    os.remove(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--bp", type=int, default=1_000_000_000)
    ap.add_argument("--many-contigs", type=int, default=200_000)
    ap.add_argument("--many-bp", type=int, default=260_000_000)
    ap.add_argument("--many-reads", type=int, default=2_400_000)
    ap.add_argument("--limit", type=int, default=600, help="time limit of one run of the binary, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_runs_device.json"))
    a = ap.parse_args()
    out = {"what": "depth runs: COV_K_DEPTH_RUNS and the arena pass per chunk, runs emitted, wall time of `coverm-amd depth`, beside Session.depth per target + numpy RLE (tools/depth_runs_probe.py)",
           "peak_hbm_tb_per_s": 8.0}
    with tempfile.TemporaryDirectory() as tmp:
        out["config2"] = one_sample("config2", a.contigs, a.bp, a.reads, 1, tmp, a.limit)
        out["many_contigs"] = one_sample("many_contigs", a.many_contigs, a.many_bp, a.many_reads, 21, tmp, a.limit, min_len=1000, max_len=40_000)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "chunks"} if isinstance(v, dict) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
