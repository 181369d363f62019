"""Start-up cost of genomes defined by FASTA files (`coverm genome -d`), written to profiles/genome_fasta_resolution.json.

    python tools/genome_fasta_probe.py resolve [--files 20000] [--contigs 2000000] [--gbytes 6] [--threads 8 16] [--dir /dev/shm/...]
        covh_genome_set_from_fasta over synthetic plain FASTA files read from the page cache (each file read once first):
        median of five resolutions per thread count.  CPU only.
    python tools/genome_fasta_probe.py e2e [--runs 5]
        config 3 at 20 M reads (2 000 contigs, 500 genome files): the coverm-amd binary with -d and with the equivalent
        --genome-definition, runs alternated, median wall of each.  Needs the GPU.

Each mode replaces its own section of the JSON file and keeps the other.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "genome_fasta_resolution.json")


def save(section, data):
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc[section] = data
    with open(OUT, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({section: data}, indent=1))


def machine():
    cpu = ""
    if os.path.exists("/proc/cpuinfo"):
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    return {"cpu": cpu, "cpus_available": len(os.sched_getaffinity(0)), "gpu_visible": os.path.exists("/dev/kfd")}


def resolve(a):
    from coverm_amd import host
    d = a.dir
    os.makedirs(d, exist_ok=True)
    per_file = a.contigs // a.files
    seq_per_contig = int(a.gbytes * 1e9 / a.contigs)
    line = b"ACGTTGCAAGGCTTAACCGGTATACGCGATATCCGGAATTCCGGTTAACCGGTTACGATCGATCGTAGCTAGCTAGCATCGATCG\n"   # 80 bases + newline
    body = (line * (seq_per_contig // len(line) + 1))[:seq_per_contig]
    if not body.endswith(b"\n"):
        body = body[:-1] + b"\n"
    t0 = time.time()
    paths = []
    for f in range(a.files):
        p = os.path.join(d, "bin%05d.fna" % f)
        paths.append(p)
        if os.path.exists(p) and os.path.getsize(p) == per_file * (len(b">b%05d_c%07d desc\n" % (0, 0)) + len(body)):
            continue
        with open(p, "wb") as fh:
            fh.write(b"".join(b">b%05d_c%07d desc\n" % (f, k) + body for k in range(per_file)))
    total = sum(os.path.getsize(p) for p in paths)
    for p in paths:                      # page cache
        with open(p, "rb") as fh:
            while fh.read(1 << 24):
                pass
    t_write = time.time() - t0
    res = {}
    for t in a.threads:
        times = []
        for _ in range(5):
            t1 = time.perf_counter()
            gs = host.GenomeSet(paths, threads=t)
            times.append(time.perf_counter() - t1)
            n = len(gs.genomes)
            del gs
        res["threads_%d" % t] = {"median_s": round(statistics.median(times), 4), "runs_s": [round(x, 4) for x in times]}
        print("threads %d: median %.3f s (%s)" % (t, statistics.median(times), ", ".join("%.3f" % x for x in times)), flush=True)
    save("resolve", {"files": a.files, "contigs": per_file * a.files, "bytes": total, "genomes": n, "page_cache": True,
                     "what": "covh_genome_set_from_fasta wall (read, scan, table); the binary fills its contig -> genome map beside "
                             "the device sessions' start-up on top of this",
                     "machine": machine(), "setup_s": round(t_write, 1), **res})
    if a.clean:
        shutil.rmtree(d)


def e2e(a):
    from coverm_amd import bam as cbam
    from coverm_amd import synth
    from tests import binary
    ref = synth.make_reference(2000, 400_000_000, seed=1)
    batch = synth.make_reads(ref, 20_000_000, seed=2)
    d = a.dir
    os.makedirs(d, exist_ok=True)
    bam = os.path.join(d, "config3_20M.bam")
    cbam.write_bam(bam, ref.names, ref.lengths, batch, with_seq=2, threads=16)
    gdir = os.path.join(d, "genomes")
    os.makedirs(gdir, exist_ok=True)
    per, rows = {}, []
    for i, n in enumerate(ref.names):
        if i % 11 != 3:
            per.setdefault("bin%03d" % (i % 500), []).append(n)
    for g in sorted(per):
        with open(os.path.join(gdir, g + ".fna"), "w") as fh:
            fh.write("".join(">%s\n%s\n" % (n, "ACGT" * 20) for n in per[g]))
        rows += ["%s\t%s\n" % (g, n) for n in per[g]]
    defn = os.path.join(d, "genomes.tsv")
    with open(defn, "w") as fh:
        fh.write("".join(rows))
    base = binary.argv("genome", [bam], threads=16, methods=["relative_abundance", "rpkm", "tpm"])
    legs = {"genome_definition": base + ["--genome-definition", defn], "fasta_directory": base + ["-d", gdir]}
    times = {k: [] for k in legs}
    outs = {}
    for r in range(a.runs + 1):                 # the first round warms the page cache and the runtime
        for k, argv in legs.items():
            time.sleep(1.0)
            t0 = time.perf_counter()
            p = subprocess.run(argv, capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                sys.exit("%s failed: %s" % (k, p.stderr[-2000:]))
            outs[k] = p.stdout
            if r:
                times[k].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    save("e2e_config3", {"reads": 20_000_000, "contigs": 2000, "genome_files": len(per), "threads": 16, "outputs_identical": outs["genome_definition"] == outs["fasta_directory"],
                         "median_s": {k: round(v, 4) for k, v in med.items()}, "runs_s": {k: [round(x, 4) for x in v] for k, v in times.items()},
                         "fasta_minus_definition_s": round(med["fasta_directory"] - med["genome_definition"], 4), "machine": machine()})
    shutil.rmtree(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["resolve", "e2e"])
    ap.add_argument("--files", type=int, default=20000)
    ap.add_argument("--contigs", type=int, default=2_000_000)
    ap.add_argument("--gbytes", type=float, default=6.0)
    ap.add_argument("--threads", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--clean", action="store_true")
    a = ap.parse_args()
    if a.dir is None:
        a.dir = os.path.join("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp", "coverm_amd_fasta_probe_%d" % os.getpid())
    resolve(a) if a.mode == "resolve" else e2e(a)


if __name__ == "__main__":
    main()
