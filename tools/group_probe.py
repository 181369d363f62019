"""Measures cov_group_records (COV_K_GROUP) on one MI355X and writes profiles/group_records.json.

    python tools/group_probe.py [--reads 50000000] [--bench-ab FILE.jsonl] [-o profiles/group_records.json]

Per contig count (5 000, 200 000, 2 000 000): synthetic records (150M CIGARs, one word each; tids drawn uniformly), randomly permuted and
already grouped; COV_K_GROUP milliseconds (median of three sessions) and its split — order check / sort passes / gather — as the library
prints it under COVERM_CLI_TIMING; beside them the algorithmic bytes of what runs and bytes / time against 8 TB/s.
--bench-ab: lines {"side": "parent" | "branch", "line": <bench.py's JSON line>} of alternated `python bench.py --gpus 1 --steps 20 --warmup 3`
runs on one box (the guard that the default path did not get slower); both series are copied into the same file."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

os.environ["COVERM_CLI_TIMING"] = "1"      # read once when the library loads
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from coverm_amd.engine import FilterConfig, RecordBatch, Session  # noqa: E402

HBM = 8e12
SPLIT = re.compile(r"\[covermhip\] group: (\d+) records, (\d+) passes, (\d+) moved; order check ([\d.]+) ms, sort ([\d.]+) ms, gather ([\d.]+) ms")


def records(n, n_contigs, seed):
    rng = np.random.default_rng(seed)
    tid = np.sort(rng.integers(0, n_contigs, n, dtype=np.int32))
    z8 = np.zeros(n, np.uint8)
    return RecordBatch(tid, rng.integers(0, 1000, n, dtype=np.int32), np.zeros(n, np.uint16), z8 + 60, np.zeros(n, np.uint32), z8 + 1, np.full(n, 150, np.uint32),
                       np.arange(n + 1, dtype=np.uint32), np.full(n, (150 << 4), np.uint32))


def take(b, perm):
    return RecordBatch(b.tid[perm], b.pos[perm], b.flag, b.mapq, b.nm, b.nm_kind, b.l_seq, b.cigar_off, b.cigar)      # (the other columns are constant)


def one(batch, lens, log):
    with Session(0, FilterConfig(), 75) as s:
        s.set_targets(lens)
        s.push(batch)
        log.seek(0, 2)
        at = log.tell()
        moved = s.group_records()
        ms, launches = s.group_kernel_ms()
        log.seek(at)
        m = SPLIT.search(log.read())
    split = dict(order_check_ms=float(m.group(4)), sort_ms=float(m.group(5)), gather_ms=float(m.group(6)), passes=int(m.group(2))) if m else None
    return dict(ms=ms, launches=launches, moved=moved, split=split)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--bench-ab")
    ap.add_argument("-o", "--output", default=os.path.join(ROOT, "profiles", "group_records.json"))
    a = ap.parse_args()
    log = tempfile.TemporaryFile(mode="w+")
    os.dup2(log.fileno(), 2)
    out = {"reads": a.reads, "hbm_bytes_per_s": HBM, "cases": []}
    for n_contigs in (5_000, 200_000, 2_000_000):
        lens = np.full(n_contigs, 2000, np.int64)
        b = records(a.reads, n_contigs, 1)
        perm = np.random.default_rng(2).permutation(a.reads)
        for shape, batch in (("random", take(b, perm)), ("grouped", b)):
            runs = [one(batch, lens, log) for _ in range(3)]
            r = sorted(runs, key=lambda x: x["ms"])[1]
            n, ncig = a.reads, a.reads
            passes = r["split"]["passes"] if r["split"] else 0
            # what runs: the check reads tid; pass 0 reads tid twice and writes key (unless it is the last) + index; a later pass reads the key twice
            # and the index once and writes index (+ key unless last); the gather reads and writes 24 B per record + the CIGAR words + 4 B of order
            by = dict(order_check=4 * n)
            if r["moved"]:
                by["sort"] = sum(4 * n * (2 + (0 if p == 0 else 1) + 1 + (0 if p == passes - 1 else 1)) for p in range(passes))
                by["gather"] = 2 * (24 * n + 4 * ncig) + 4 * n
            total = sum(by.values())
            out["cases"].append(dict(n_contigs=n_contigs, input=shape, group_ms_runs=[x["ms"] for x in runs], group_ms=r["ms"], launches=r["launches"], moved=r["moved"],
                                     split=r["split"], algorithmic_bytes=by, algorithmic_bytes_total=total, frac_of_8TBps=total / (r["ms"] * 1e-3) / HBM if r["ms"] else None))
            print(json.dumps(out["cases"][-1]), flush=True)
    if a.bench_ab:
        series = {"parent": [], "branch": []}
        for line in open(a.bench_ab):
            d = json.loads(line)
            series[d["side"]].append(d["line"]["ms_per_step"])
        out["bench_guard"] = {k: dict(ms_per_step=v, median=statistics.median(v), spread=max(v) - min(v)) for k, v in series.items()}
        out["bench_guard"]["branch_within_parent_spread"] = abs(out["bench_guard"]["branch"]["median"] - out["bench_guard"]["parent"]["median"]) <= out["bench_guard"]["parent"]["spread"]
    with open(a.output, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
