"""`coverm-amd genome -s '~' -m trimmed_mean variance covered_fraction` of this tree against the binary of another build (the parent
commit's), alternating, one process per run (COVERM_NO_FAST_EXIT=1), with the COVERM_CLI_TIMING split, the bytes each side fetches per
sample and the HIP-event times of the kernels that build the entry table (cov_kernel_ms, COV_K_SEP) and of the genome kernels behind them
(COV_K_GENOME).  The method of tools/genome_device_probe.py.  Writes profiles/genome_separator_device.json.

    python tools/separator_device_probe.py --parent /path/to/parent/coverm_amd/coverm-amd [--reads 50000000] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from coverm_amd import bam as cbam, synth
from coverm_amd.engine import FilterConfig, Session
from coverm_amd.host import CoverageEstimator as E

CUR = os.path.join(ROOT, "coverm_amd", "coverm-amd")
ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="coverm-amd binary of the build to compare with (its libcovermhip.so beside it)")
ap.add_argument("--reads", type=int, default=50_000_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genome_separator_device.json"))
ap.add_argument("--only", type=int, default=None, help="index of the one config to run (0: 5 000 contigs, 1: 200 000, 2: 2 000 000)")
args = ap.parse_args()
PAR = args.parent
N_READS = args.reads
CONFIGS = [("5000_contigs_500_genomes", 5000, 500), ("200000_contigs_2000_genomes", 200_000, 2000), ("2000000_contigs_20000_genomes", 2_000_000, 20_000)]
OUT = args.out
METHODS = ["trimmed_mean", "variance", "covered_fraction"]
res = {"reads": N_READS, "methods": METHODS, "separator": "~", "runs_per_side": 5,
       "order": "parent, branch alternating; one process per run, COVERM_NO_FAST_EXIT=1", "configs": []}
if os.path.exists(OUT) and args.only is not None:      # one config per call: the file collects them
    res = json.load(open(OUT))
    res["configs"] = [c for c in res["configs"] if c["name"] != CONFIGS[args.only][0]]


def run(binary, bam, extra_env=None):
    env = dict(os.environ, COVERM_NO_FAST_EXIT="1", COVERM_CLI_TIMING="1", **(extra_env or {}))
    t0 = time.perf_counter()
    r = subprocess.run([binary, "genome", "-b", bam, "-s", "~", "-m"] + METHODS + ["-t", "16"], capture_output=True, text=True, timeout=240, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-2000:]); raise SystemExit("run failed: %d" % r.returncode)
    d = {"wall_s": round(wall, 4), "table_sha1": hashlib.sha1(r.stdout.encode()).hexdigest()[:12]}
    m = re.search(r"finish\+fetch ([0-9.]+)s", r.stderr); d["finish_fetch_s"] = float(m.group(1)) if m else None
    m = re.search(r"scan drivers ([0-9.]+)s", r.stderr); d["scan_drivers_s"] = float(m.group(1)) if m else None
    m = re.search(r"histogram fetch: (\d+) bins, (\d+) bytes", r.stderr); d["hist_bytes"] = int(m.group(2)) if m else None
    m = re.search(r"separator entries from the device \(cov_set_genome_runs\): (\d+) entries x \d+ estimators, (\d+) bytes", r.stderr)
    d["entries"], d["entry_bytes"] = (int(m.group(1)), int(m.group(2))) if m else (None, None)
    m = re.search(r"genome ids to the device \(cov_set_genome_runs\) \d+ ids, ([0-9.]+)s", r.stderr); d["genome_ids_s"] = float(m.group(1)) if m else None
    m = re.search(r"open ([0-9.]+)s, ingest", r.stderr); d["open_s"] = float(m.group(1)) if m else None
    return d


for name, n_contigs, n_genomes in (CONFIGS if args.only is None else [CONFIGS[args.only]]):
    t0 = time.time()
    per = n_contigs // n_genomes
    ref = synth.make_reference(n_contigs, 1_000_000_000 if n_contigs <= 5000 else 3_000_000_000, seed=1, contigs_per_genome=per, min_len=400 if n_contigs > 5000 else 2000)
    batch = synth.make_reads(ref, N_READS, seed=2)
    bam = "/dev/shm/coverm_amd_measure_%d.bam" % os.getpid()
    try:
        cbam.write_bam(bam, ref.names, ref.lengths, batch, with_seq=2, threads=16)
        print(name, "sample written in %.0fs" % (time.time() - t0), flush=True)
        c = {"name": name, "contigs": n_contigs, "genomes": n_genomes, "parent": [], "branch": []}
        run(PAR, bam); run(CUR, bam)      # warm the page cache and both binaries
        for k in range(5):
            c["parent"].append(run(PAR, bam)); c["branch"].append(run(CUR, bam))
            print(name, k, c["parent"][-1]["wall_s"], c["branch"][-1]["wall_s"], flush=True)
        host = run(CUR, bam, {"COVERM_HOST_ESTIMATES": "1"})
        assert len({r["table_sha1"] for r in c["parent"] + c["branch"] + [host]}) == 1, "tables differ"
        assert all(r["entry_bytes"] for r in c["branch"]) and not any(r["entry_bytes"] for r in c["parent"] + [host]), "a side took the other path"
        for side in ("parent", "branch"):
            w = [r["wall_s"] for r in c[side]]
            c[side + "_median_wall_s"] = statistics.median(w); c[side + "_spread_s"] = round(max(w) - min(w), 4)
            c[side + "_median_finish_fetch_s"] = statistics.median([r["finish_fetch_s"] for r in c[side]])
            c[side + "_median_scan_drivers_s"] = statistics.median([r["scan_drivers_s"] for r in c[side]])
            c[side + "_median_open_s"] = statistics.median([r["open_s"] for r in c[side]])
        c["branch_median_genome_ids_s"] = statistics.median([r["genome_ids_s"] for r in c["branch"]])
        block = n_contigs * 160
        c["bytes_fetched_per_sample"] = {
            "parent": block + (host["hist_bytes"] or 0), "branch": c["branch"][0]["entry_bytes"], "branch_entries": c["branch"][0]["entries"],
            "parent_per_contig_block": block, "parent_histogram": host["hist_bytes"],
            "how": "parent: DERIVED, not logged by the parent's binary — 160 B x contigs (the DevContig block every cov_finish copies) + the histogram bytes this "
                   "tree's host path (COVERM_HOST_ESTIMATES=1, the parent's code path) reports for the same file; branch: logged by the run (cov_finish_genomes "
                   "copies no per-contig block), plus the 4 kB of device-wide counters both sides copy and the 16 bytes of the table's counts"}
        # HIP-event time of the new kernels, in process, same records: the table (COV_K_SEP: k_sep_*) and the genome kernels over it (COV_K_GENOME)
        est = [E.new_estimator_trimmed_mean(0.05, 0.95, 0.1, 75), E.new_estimator_variance(0.1, 75), E.new_estimator_covered_fraction(0.1)]
        with Session(0, FilterConfig(), 75, want_hist=True) as s:
            s.set_targets(ref.lengths); s.set_genome_runs(ref.genome_of_contig, n_genomes); s.set_estimators(est); s.push(batch)
            sep, gen, wall = [], [], []
            for _ in range(4):
                t1 = time.perf_counter(); s.finish_genomes(); wall.append(round((time.perf_counter() - t1) * 1e3, 4))
                sep.append(round(s.sep_kernel_ms()[0], 4)); gen.append(round(s.genome_kernel_ms()[0], 4))
            c["sep_table_kernels_hip_event_ms"] = sep[1:]; c["genome_kernels_hip_event_ms"] = gen[1:]; c["finish_genomes_wall_ms"] = wall[1:]
            c["entries_in_process"] = s.genome_entry_count()
            c["all_kernels_ms"] = {k: round(v[0], 4) for k, v in s.kernel_ms().items() if v[1]}
        # ... the same finish with the table fixed by the header (cov_set_genomes over the same genomes): what the scans, the compaction and
        # the table's one synchronisation add to a finish
        with Session(0, FilterConfig(), 75, want_hist=True) as s:
            s.set_targets(ref.lengths); s.set_genomes(ref.genome_of_contig, n_genomes); s.set_estimators(est); s.push(batch)
            wall = []
            for _ in range(4):
                t1 = time.perf_counter(); s.finish_genomes(); wall.append(round((time.perf_counter() - t1) * 1e3, 4))
            c["finish_genomes_wall_ms_contig_names_table"] = wall[1:]
        res["configs"].append(c)
        json.dump(res, open(OUT, "w"), indent=1)
    finally:
        if os.path.exists(bam): os.remove(bam)
    del batch
print(json.dumps({c["name"]: (c["parent_median_wall_s"], c["branch_median_wall_s"]) for c in res["configs"]}))
