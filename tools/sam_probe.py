"""SAM text route, measured: device decode (COV_K_SAM) and end-to-end wall time through the binary, from a file and from a pipe.

    python tools/sam_probe.py --reads 2000000 --contigs 5000 [--read-len 150] [--parent /path/to/parent/coverm-amd] [--parent-timeout 600] [--timeout 600]
                              [--out profiles/sam_device_decode.json]

Writes (appends a case to) the JSON file: bytes, records, COV_K_SAM time and the implied GB/s, the driver's own split (read, slot waits,
feed calls), wall time of `coverm-amd contig -m mean` on the SAM file and on `cat file |`, and — with --parent — the same command through
another build's binary (the whole-file host route of the commit before this route existed), stopped after --parent-timeout seconds.
Every run of the binary has a time limit and a process group of its own; the first run that fails, is killed or is stopped ends the probe,
which writes what it has measured and starts nothing more.
The text is written by a vectorised generator (fixed-width fields, one CIGAR word per read, reads sorted by reference)."""
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


def write_sam(path, n_reads, n_contigs, read_len, seed=1):
    """Sorted synthetic SAM: every line has the same width, so the whole body is one (n_reads, width) byte matrix filled column-wise."""
    rng = np.random.default_rng(seed)
    clen = 200_000
    tid = np.sort(rng.integers(0, n_contigs, n_reads))
    pos = rng.integers(1, clen - read_len, n_reads)
    tmpl = ("r%011d\t0\tctg%07d\t%07d\t60\t%dM\t*\t0\t0\t" % (0, 0, 0, read_len)).encode()
    tail = b"\tNM:i:1\tAS:i:100\n"
    width = len(tmpl) + 2 * read_len + 1 + len(tail)
    with open(path, "wb") as f:
        f.write(b"@HD\tVN:1.6\tSO:coordinate\n")
        for lo in range(0, n_contigs, 100_000):
            f.write("".join("@SQ\tSN:ctg%07d\tLN:%d\n" % (c, clen) for c in range(lo, min(n_contigs, lo + 100_000))).encode())
        for lo in range(0, n_reads, 1 << 20):
            hi = min(n_reads, lo + (1 << 20))
            m = np.empty((hi - lo, width), np.uint8)
            m[:, :len(tmpl)] = np.frombuffer(tmpl, np.uint8)

            def digits(col, w, v):
                for k in range(w):
                    m[:, col + w - 1 - k] = 48 + (v // 10 ** k) % 10
            digits(1, 11, np.arange(lo, hi))
            digits(18, 7, tid[lo:hi])
            digits(26, 7, pos[lo:hi])
            a = len(tmpl)
            m[:, a:a + read_len] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (hi - lo, read_len))]
            m[:, a + read_len] = 9
            m[:, a + read_len + 1:a + 2 * read_len + 1] = rng.integers(35, 74, (hi - lo, read_len))
            m[:, a + 2 * read_len + 1:] = np.frombuffer(tail, np.uint8)
            f.write(m.tobytes())
    return os.path.getsize(path)


class Stop(Exception):
    """A run failed, was killed or ran out of time: nothing more is started on the device."""


def wall(argv, stdin_path=None, timeout=600.0):
    """One run of the binary in a process group of its own, under its own time limit.  A run that does not end with status 0 — a non-zero
    status, a signal, the time limit (the whole group is killed) — raises Stop with what is known of it."""
    t0 = time.time()
    cat = subprocess.Popen(["cat", stdin_path], stdout=subprocess.PIPE) if stdin_path else None
    child = subprocess.Popen(argv, stdin=cat.stdout if cat else subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True)
    if cat:
        cat.stdout.close()
    try:
        out, err = child.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(child.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        child.communicate()
        raise Stop({"stopped_after_s": timeout})
    finally:
        if cat:
            cat.kill()
            cat.wait()
    r = {"wall_s": round(time.time() - t0, 3), "returncode": child.returncode, "stdout_bytes": len(out)}
    if child.returncode != 0:
        r["stderr_tail"] = err.decode(errors="replace")[-500:]
        raise Stop(r)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-timeout", type=float, default=600)
    ap.add_argument("--timeout", type=float, default=600, help="time limit of each run on the new route, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_device_decode.json"))
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    from coverm_amd.engine import FilterConfig, Session
    binary = os.path.join(ROOT, "coverm_amd", "coverm-amd")
    with tempfile.TemporaryDirectory(dir=a.tmp) as d:
        p = os.path.join(d, "s.sam")
        nbytes = write_sam(p, a.reads, a.contigs, a.read_len)
        case = {"reads": a.reads, "contigs": a.contigs, "read_len": a.read_len, "bytes": nbytes}
        with Session(0, FilterConfig(), 75) as s:
            for _ in range(2):                       # the second ingest: buffers and the page cache are warm
                s.reset()
                _, _, n, t = s.sam_ingest(p)
                ms, launches = s.sam_kernel_ms()
            case.update(records=n, cov_k_sam_ms=round(ms, 3), launches=launches, decode_GBps=round(nbytes / ms / 1e6, 2), driver_s=t,
                        ingest_GBps=round(nbytes / t["total"] / 1e9, 3))
        argv = [binary, "contig", "-m", "mean", "-b"]
        # every run has its own limit; the first one that fails, is killed or runs out of time ends the probe (what was measured is
        # written).  The runs that may be stopped — the host route, the parent — come last.
        runs = [("file", argv + [p], None, a.timeout)] * 3 + [("pipe", argv + ["-"], p, a.timeout)] * 3 + [("host_route", argv + [p, "--no-stream"], None, a.parent_timeout)]
        if a.parent:
            runs.append(("parent", [a.parent, "contig", "-m", "mean", "-b", p], None, a.parent_timeout))
        for key, v, stdin_path, limit in runs:
            try:
                case.setdefault(key, []).append(wall(v, stdin_path, limit))
            except Stop as e:
                case.setdefault(key, []).append(e.args[0])
                case["ended_at"] = key
                break
    doc = {"cases": []}
    if os.path.exists(a.out):
        doc = json.load(open(a.out))
    doc["cases"].append(case)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(case))


if __name__ == "__main__":
    main()
