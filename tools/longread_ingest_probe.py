"""How long the device ingest takes on a long-read BAM as a long-read pipeline writes it (dorado / minimap2: NM first, MD:Z, MM:Z, ML:B,C,
SA:Z on a tenth of the reads, thousands of CIGAR operations per record), on this build and on another one (the parent commit's, built in
a checkout of its own), alternating on one box.

    python tools/longread_ingest_probe.py --other /path/to/parent/checkout [--runs 5] [--out profiles/longread_device_ingest.json]
                                          [--kernel-figures FILE]      (register / LDS figures per kernel, JSON, copied into the output)
                                          [--bench-lines FILE]         (the bench.py result lines of both builds, JSON, copied into the output)

The sample: synth.make_long_reads(ref, 20 000, mean_len=20 000) over a 40-contig reference, written by the small BAM writer below (the
project's writers emit NM only).  Every measurement is a process of its own that ingests the file twice into a fresh session and reports
covh_bam_gpu_ingest's timing[3] (total seconds, host clock around the ingest including its last synchronise) of the second pass, so that
code loading and first allocations are not in the figure; the streamed CPU reader is timed once for scale."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the sample
def digits(n, rng):
    return (rng.integers(0, 10, n, dtype=np.uint8) + 48).tobytes()


def write_sample(path, n_reads=20_000, mean_len=20_000, seed=29):
    sys.path.insert(0, ROOT)
    from coverm_amd import synth
    ref = synth.make_reference(40, 600_000_000, seed=18, min_len=2_000_000, max_len=40_000_000)
    b = synth.make_long_reads(ref, n_reads, seed=seed, mean_len=mean_len)
    rng = np.random.default_rng(seed)
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", len(ref.names))
    for name, length in zip(ref.names, ref.lengths):
        head += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", int(length))
    with open(path, "wb") as out:
        pend = [head]
        size = len(head)

        def flush(everything):
            nonlocal pend, size
            data = b"".join(pend)
            q = 0
            while len(data) - q >= 0xff00 or (everything and q < len(data)):
                chunk = data[q:q + 0xff00]
                co = zlib.compressobj(1, zlib.DEFLATED, -15)
                comp = co.compress(chunk) + co.flush()
                out.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
                q += len(chunk)
            pend, size = [data[q:]], len(data) - q
        for i in range(b.n_records):
            l_seq = int(b.l_seq[i])
            cigar = b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])]
            if len(cigar) > 65_535:
                raise SystemExit("a CIGAR of more than 65535 operations: not what this sample is about")
            aux = b"NMI" + struct.pack("<I", int(b.nm[i])) + b"MDZ" + digits(l_seq // 10, rng) + b"\0" + b"MMZ" + digits(l_seq // 8, rng) + b"\0"
            aux += b"MLBC" + struct.pack("<I", l_seq // 10) + rng.integers(0, 256, l_seq // 10, dtype=np.uint8).tobytes()
            if i % 10 == 0:
                aux += b"SAZ" + b"%s,%d,+,%dS%dM,60,%d;" % (ref.names[0].encode(), 1 + i, l_seq // 2, l_seq // 2, i % 50) + b"\0"
            name = b"read-%08d" % i
            core = struct.pack("<iiBBHHHiiii", int(b.tid[i]), int(b.pos[i]), len(name) + 1, int(b.mapq[i]), 4680, len(cigar), int(b.flag[i]), l_seq, -1, -1, 0)
            body = core + name + b"\0" + np.asarray(cigar, np.uint32).tobytes() + rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes() + (rng.integers(0, 42, l_seq, dtype=np.uint8)).tobytes() + aux
            pend.append(struct.pack("<i", len(body)) + body)
            size += 4 + len(body)
            if size >= 64 * 0xff00:
                flush(False)
        flush(True)
        out.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    return b.n_records


# ------------------------------------------------------------------------------------------------ one measurement (a process of its own)
def one(root, path, what):
    sys.path.insert(0, root)
    from coverm_amd import bam as cbam
    from coverm_amd.engine import FilterConfig, Session
    if what == "cpu":
        t0 = time.perf_counter()
        n = sum(x.n_records for x in list(cbam.stream_batches(path, 16))[1:])
        print(json.dumps({"seconds": time.perf_counter() - t0, "records": n}))
        return
    res = {}
    with Session(0, FilterConfig(), 75) as s:
        for rep in range(2):
            s.reset()
            try:
                _, _, n, timing = cbam.gpu_ingest(s, path, threads=16)
                res = {"seconds": timing["total"] if isinstance(timing, dict) else float(timing[3]), "records": int(n), "route": "device ingest"}
            except cbam.IngestFallback as e:
                res = {"seconds": None, "records": 0, "route": "handed to the CPU reader: " + str(e)}
            if hasattr(cbam, "ingest_stats"):
                res["stats"] = cbam.ingest_stats(s)
    print(json.dumps(res))


def child(root, path, what):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, "--root", root, "--sample", path], capture_output=True, text=True, timeout=900, cwd=root)
    if r.returncode != 0:
        raise SystemExit("measurement failed in %s: %s" % (root, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="checkout of the build to compare with (built)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reads", type=int, default=20_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "longread_device_ingest.json"))
    ap.add_argument("--kernel-figures")
    ap.add_argument("--bench-lines")
    ap.add_argument("--sample")
    ap.add_argument("--one")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    if a.one:
        return one(a.root, a.sample, a.one)
    tmp = tempfile.mkdtemp(prefix="longread_probe_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = a.sample or os.path.join(tmp, "longreads.bam")
    try:
        t0 = time.time()
        n = write_sample(path, a.reads) if not a.sample else None
        print("sample: %s, %.1f MB, %s records, written in %.1fs" % (path, os.path.getsize(path) / 1e6, n, time.time() - t0), flush=True)
        sides = [("parent", os.path.abspath(a.other))] if a.other else []
        sides.append(("branch", ROOT))
        runs = {k: [] for k, _ in sides}
        last = {}
        for i in range(a.runs):
            for k, root in sides:
                r = child(root, path, "gpu")
                runs[k].append(r["seconds"])
                last[k] = r
                print("run %d %s: %s" % (i, k, json.dumps(r)), flush=True)
        cpu = child(ROOT, path, "cpu")
        print("streamed CPU reader: %s" % json.dumps(cpu), flush=True)
        res = {"sample": {"reads": a.reads, "mean_len": 20_000, "contigs": 40, "file_bytes": os.path.getsize(path), "records": cpu["records"],
                          "tags": "NM:I first, MD:Z l_seq/10, MM:Z l_seq/8, ML:B,C l_seq/10, SA:Z on a tenth"},
               "what": "covh_bam_gpu_ingest timing[3] (total seconds) of the second ingest of a process, builds alternating on one box",
               "seconds": runs, "route": {k: last[k]["route"] for k in last}, "streamed_cpu_reader_s": cpu["seconds"]}
        for k, v in runs.items():
            if all(x is not None for x in v):
                res["median_" + k] = float(np.median(v))
                res["spread_" + k] = max(v) - min(v)
        if "stats" in last.get("branch", {}):
            res["branch_stats"] = last["branch"]["stats"]
        for key, f in (("kernel_figures", a.kernel_figures), ("bench_lines", a.bench_lines)):
            if f:
                res[key] = json.load(open(f))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        print(json.dumps(res))
    finally:
        if not a.sample and os.path.exists(path):
            os.remove(path)
        try:
            os.rmdir(tmp)
        except OSError:
            pass


if __name__ == "__main__":
    main()
