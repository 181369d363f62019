"""What `coverm-amd contig --gff` behind the device ingest costs with the per-gene read aggregates computed on the device
(cov_interval_reads_compute: 32 bytes per gene come back) and with the records copied back for the host's record pass
(COVERM_GENE_READS_ON_HOST=1: 24 bytes per record and every CIGAR word — what the binary did before), alternating on one box.

    python tools/gene_reads_probe.py [--reads 20000000] [--contigs 5000] [--genes 50000] [--runs 5] [--out profiles/gene_reads_device.json]

The sample: a synthetic sorted BAM (synth.make_reads over a reference of --contigs contigs, written by the project's BAM writer) and a GFF of
--genes genes spread over the contigs.  Every run is one process of the binary (`-m mean count anir`, COVERM_CLI_TIMING=1) with a time limit;
its wall time is the figure.  The output holds both routes' times, medians and ranges, the COV_K_GENE_READS milliseconds the device route
reports, the bytes each route fetches for the read aggregates, one timing line of each route, and the rule's verdict: the device route
stays the default if its median is not above the host route's median by more than the host runs' own max - min."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_sample(d, n_reads, n_contigs, n_genes, seed=61):
    from coverm_amd import bam as cbam
    from coverm_amd import synth
    ref = synth.make_reference(n_contigs, 100_000 * n_contigs, seed=seed, min_len=1500, max_len=2_000_000)
    batch = synth.make_reads(ref, n_reads, seed=seed + 1)
    path = os.path.join(d, "genes.bam")
    cbam.write_bam(path, ref.names, ref.lengths, batch, with_seq=1, threads=16)
    rng = np.random.default_rng(seed + 2)
    lens = np.asarray(ref.lengths, np.int64)
    per = np.maximum(1, np.round(n_genes * lens / lens.sum()).astype(np.int64))
    gff = os.path.join(d, "genes.gff")
    n = 0
    with open(gff, "w") as fh:
        fh.write("##gff-version 3\n")
        for name, L, k in zip(ref.names, lens, per):
            starts = np.sort(rng.integers(1, max(2, L - 1), k))
            for j, s in enumerate(starts):
                fh.write("%s\tsyn\tgene\t%d\t%d\t.\t+\t.\tID=%s_g%d\n" % (name, s, min(L, s + int(rng.integers(100, 3000))), name.replace("~", "_"), j))
                n += 1
    cigar_words = int(batch.cigar_off[-1]) - int(batch.cigar_off[0])
    return path, gff, batch.n_records, cigar_words, n


def one_run(path, gff, on_host, limit):
    from tests import binary
    env = dict(os.environ, COVERM_CLI_TIMING="1")
    env.pop("COVERM_GENE_READS_ON_HOST", None)
    if on_host:
        env["COVERM_GENE_READS_ON_HOST"] = "1"
    t0 = time.perf_counter()
    r = subprocess.run(binary.argv("contig", [path], methods=["mean", "count", "anir"], gff=gff, threads=16), capture_output=True, text=True, env=env, timeout=limit)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("the binary failed: %s" % r.stderr[-2000:])
    line = [ln for ln in r.stderr.splitlines() if "--gff over the device ingest" in ln]
    if not line:
        raise SystemExit("no --gff timing line: the run did not take the device ingest\n%s" % r.stderr[-2000:])
    lib = [ln for ln in r.stderr.splitlines() if "[covermhip] interval reads" in ln]
    return dt, line[0], (lib[0] if lib else None), r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--contigs", type=int, default=5_000)
    ap.add_argument("--genes", type=int, default=50_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds one run of the binary may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gene_reads_device.json"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="gene_reads_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        t0 = time.time()
        path, gff, n_records, cigar_words, n_genes = write_sample(tmp, a.reads, a.contigs, a.genes)
        print("sample: %d records, %d genes, %.1f MB, written in %.1fs" % (n_records, n_genes, os.path.getsize(path) / 1e6, time.time() - t0), flush=True)
        secs = {"device": [], "host": []}
        lines, lib_line, text = {}, None, {}
        one_run(path, gff, False, a.limit)                      # the file into the page cache, the code objects loaded once
        for i in range(a.runs):
            for route in ("device", "host"):
                dt, line, lib, out = one_run(path, gff, route == "host", a.limit)
                secs[route].append(dt)
                lines[route] = line
                text[route] = out
                lib_line = lib if route == "device" and lib else lib_line
                print("run %d %s: %.3fs  %s" % (i, route, dt, line), flush=True)
        if text["device"] != text["host"]:
            raise SystemExit("the two routes printed different tables")
        m = re.search(r"([0-9.]+) kernels ms", lines["device"])
        med = {k: float(np.median(v)) for k, v in secs.items()}
        spread = {k: max(v) - min(v) for k, v in secs.items()}
        res = {"sample": {"reads": n_records, "contigs": a.contigs, "genes": n_genes, "cigar_words": cigar_words, "file_bytes": os.path.getsize(path)},
               "what": "wall seconds of one `coverm-amd contig --gff -m mean count anir` process, routes alternating on one box, after one warming run",
               "seconds": secs, "median_s": med, "range_s": {k: [min(v), max(v)] for k, v in secs.items()}, "spread_s": spread,
               "gene_reads_kernels_ms": float(m.group(1)) if m else None,
               "bytes_fetched_for_read_aggregates": {"device": 32 * n_genes, "host": 24 * n_records + 4 + 4 * cigar_words},
               "timing_line": lines, "library_line": lib_line,
               "rule": "the device route stays the default if median_s.device <= median_s.host + spread_s.host",
               "device_route_is_default": bool(med["device"] <= med["host"] + spread["host"])}
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res))
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
