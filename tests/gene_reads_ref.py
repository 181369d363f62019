"""The per-gene read aggregates of the reference's gene scan (src/genes.rs:206-304, 493-524), restated record by record in Python for the
tests of csrc/gene_reads_core.h, cov_interval_reads_compute and covh_gene_coverage_reads.  Python floats are IEEE f64 and the running sum
below is the serial one, so sum_identity is exact; the reader stage's f32 expressions are evaluated in numpy float32, operation by
operation (filter.rs:243-279)."""
import bisect
from collections import namedtuple

import numpy as np

OK, ERR_UNSORTED, ERR_NM_MISSING, ERR_NM_BADTYPE, ERR_BAD_TID = 0, 1, 2, 3, 7
SKIP, TAKE, NM_MISSING, NM_BADTYPE = 0, 1, 2, 3
MSG_UNSORTED = "BAM file appears to be unsorted. Input BAM files must be sorted by reference (i.e. by samtools sort)"
MSG_BAD_TID = "record refers to a reference id outside the header (Corrupt BAM file?)"

Filter = namedtuple("Filter", "include_improper_pairs include_supplementary include_secondary filter_single min_mapq min_aligned_length "
                              "min_percent_identity min_aligned_percent")
F32 = np.float32


def filter_of(cfg) -> Filter:
    """From a native.CovConfig (or engine.FilterConfig: the same field names)."""
    return Filter(bool(cfg.include_improper_pairs), bool(cfg.include_supplementary), bool(cfg.include_secondary), bool(cfg.filter_single),
                  int(cfg.min_mapq), int(cfg.min_aligned_length), float(cfg.min_percent_identity), float(cfg.min_aligned_percent))


def cigar_sums(words):
    aligned = indels = 0
    for w in words:
        op, ln = int(w) & 15, int(w) >> 4
        if op in (0, 7, 8):
            aligned += ln
        elif op in (1, 2):
            aligned += ln
            indels += ln
    return aligned, indels


def classify(f: Filter, flag, mapq, nm_kind, nm, l_seq, aligned, indels):
    """(state, primary, mism, ident): genes.rs:206-304 behind the reader stage's single-read branch (filter.rs:88-116, 243-279)."""
    supp, sec, unmapped = bool(flag & 0x800), bool(flag & 0x100), bool(flag & 0x4)
    nm_state = NM_MISSING if nm_kind == 0 else NM_BADTYPE
    if f.filter_single:
        if unmapped or (not f.include_supplementary and supp) or (not f.include_secondary and sec):
            return SKIP, 0, 0, 0.0
        if f.min_mapq != 255 and (mapq < f.min_mapq or mapq == 255):
            return SKIP, 0, 0, 0.0
        if nm_kind != 1:
            return nm_state, 0, 0, 0.0
        al = aligned & 0xffffffff
        with np.errstate(divide="ignore", invalid="ignore"):
            a = F32(al)
            ok = al >= f.min_aligned_length and a / F32(l_seq) >= F32(f.min_aligned_percent) and F32(1.0) - F32(nm) / a >= F32(f.min_percent_identity)
        if not ok:
            return SKIP, 0, 0, 0.0
    if (not f.include_secondary and sec) or (not f.include_supplementary and supp) or (not f.include_improper_pairs and not flag & 0x2):
        return SKIP, 0, 0, 0.0
    if unmapped:
        return SKIP, 0, 0, 0.0
    if nm_kind != 1:
        return nm_state, 0, 0, 0.0
    primary = 0 if (supp or sec) else 1
    ident = (float(aligned) - float(nm)) / float(aligned) if primary and aligned > 0 else 0.0
    return TAKE, primary, max(0, nm - indels), ident


def classify_all(f: Filter, rec):
    """One (state, primary, mism, ident) per record of a RecordBatch-like object (numpy columns)."""
    out = []
    co = rec.cigar_off
    for i in range(len(rec.tid)):
        aligned, indels = cigar_sums(rec.cigar[int(co[i]):int(co[i + 1])])
        out.append(classify(f, int(rec.flag[i]), int(rec.mapq[i]), int(rec.nm_kind[i]), int(rec.nm[i]), int(rec.l_seq[i]), aligned, indels))
    return out


def start_of(pos):
    return int(pos) & 0xffffffffffffffff if pos < 0 else int(pos)      # pos sign-extended to u64, as the host compares it


def aggregates(f: Filter, n_targets, rec, intervals, want_identity, classes=None):
    """The scan over the records in file order: (status, message, rows, mapped_total, sorted_by_start).  rows[g] = (n_reads, mismatches,
    sum_identity, contig_taken) for intervals[g] = (tid, start, end); None when the status is an error or a start decreases inside a contig."""
    classes = classes if classes is not None else classify_all(f, rec)
    per = {}                  # tid -> [starts, pprim, pmism, pident]
    last_tid, mapped, srt = -2, 0, True
    for i, (state, primary, mism, ident) in enumerate(classes):
        if state == SKIP:
            continue
        if state != TAKE:
            return (ERR_NM_MISSING if state == NM_MISSING else ERR_NM_BADTYPE), None, None, mapped, srt
        tid = int(rec.tid[i])
        if tid != last_tid:
            if tid < last_tid:
                return ERR_UNSORTED, MSG_UNSORTED, None, mapped, srt
            if tid < 0 or tid >= n_targets:
                return ERR_BAD_TID, MSG_BAD_TID, None, mapped, srt
            last_tid = tid
            per[tid] = [[], [0], [0], [0.0]]
        v = per.setdefault(tid, [[], [0], [0], [0.0]])      # (tid == -2 on the first record: the reference's last_tid lets it through)
        st = start_of(int(rec.pos[i]))
        if v[0] and st < v[0][-1]:
            srt = False
        mapped += primary
        v[0].append(st)
        v[1].append(v[1][-1] + primary)
        v[2].append((v[2][-1] + mism) & 0xffffffffffffffff)
        v[3].append(v[3][-1] + (ident if want_identity else 0.0))
    if not srt:
        return OK, None, None, mapped, False
    rows = []
    for tid, s, e in intervals:
        v = per.get(int(tid))
        if v is None:
            rows.append((0, 0, 0.0, 0))
            continue
        lo, hi = bisect.bisect_left(v[0], int(s)), bisect.bisect_left(v[0], int(e))
        rows.append((v[1][hi] - v[1][lo], (v[2][hi] - v[2][lo]) & 0xffffffffffffffff, v[3][hi] - v[3][lo], len(v[0])))
    return OK, None, rows, mapped, True


def rows_array(rows):
    from coverm_amd import native
    out = np.zeros(len(rows), dtype=native.INTERVAL_READS_DTYPE)
    for k, r in enumerate(rows):
        out[k] = r
    return out


# ---- hand-made records of every class the scan distinguishes: (flag, mapq, nm, nm_kind, l_seq, [cigar words])
def cg(*ops):
    return [(ln << 4) | "MIDNSHP=X".index(op) for ln, op in ops]


def class_records(with_nm_errors=False):
    out = []
    for bits in range(16):                                       # every combination of unmapped / secondary / supplementary / proper pair
        flag = (0x4 if bits & 1 else 0) | (0x100 if bits & 2 else 0) | (0x800 if bits & 4 else 0) | (0x2 if bits & 8 else 0)
        out.append((flag, 30, 1, 1, 100, cg((100, "M"))))
    out += [(0x2, 30, 2, 1, 10, cg((5, "M"), (3, "I"), (5, "M"), (2, "D"))),                    # NM < indels: mism saturates at 0
            (0x2, 30, 25, 1, 10, cg((10, "M"))),                                                # NM > aligned: a negative identity
            (0x2, 30, 0, 1, 20, cg((10, "S"), (5, "H"), (3, "N"), (2, "P"))),                   # aligned == 0: identity 0, 0 / 0 in the reader stage
            (0x2, 30, 7, 1, 60, cg((4, "S"), (10, "="), (2, "X"), (3, "I"), (20, "M"), (5, "D"), (100, "N"), (8, "M"), (1, "P"), (6, "H"))),
            (0x2, 30, 2999, 1, 100000, cg((100000, "M"))),                                      # 1 - 2999 / 100000 against f32(0.97001)
            (0x2, 30, 3000, 1, 100000, cg((100000, "M"))),
            (0x2, 30, 2998, 1, 100000, cg((100000, "M"))),
            (0x2, 0, 0, 1, 50, cg((50, "M"))), (0x2, 255, 0, 1, 50, cg((50, "M"))), (0x2, 9, 0, 1, 50, cg((50, "M"))), (0x2, 10, 0, 1, 50, cg((50, "M"))),
            (0x2, 30, 0, 1, 0, cg((50, "M"))),                                                  # l_seq 0: a / 0 = inf
            (0x2, 30, 1, 1, 200, cg((30, "M"))), (0x2, 30, 3, 1, 30, cg((29, "M"))),            # aligned percent, aligned length
            (0x902, 30, 4, 1, 40, cg((40, "M"))), (0x102, 30, 4, 1, 40, cg((40, "M"))),         # not primary: counted in mism, identity 0
            (0x0, 30, 0xffffffff, 1, 40, cg((40, "M")))]                                        # the largest NM
    if with_nm_errors:
        out += [(0x2, 30, 0, 0, 50, cg((50, "M"))), (0x2, 30, 0, 2, 50, cg((50, "M"))), (0x4, 30, 0, 0, 50, cg((50, "M"))), (0x102, 30, 0, 2, 50, cg((50, "M"))),
                (0x2, 3, 0, 0, 50, cg((50, "M")))]
    return out


def batch_of(rows):
    """rows: (tid, pos, flag, mapq, nm, nm_kind, l_seq, [cigar words]) -> engine.RecordBatch"""
    from coverm_amd.engine import RecordBatch
    off, cig = [0], []
    for r in rows:
        cig += r[7]
        off.append(len(cig))
    col = lambda k: [r[k] for r in rows]      # noqa: E731
    return RecordBatch.from_arrays(col(0), col(1), col(2), col(3), np.asarray(col(4), np.uint32), col(5), np.asarray(col(6), np.uint32), off,
                                   np.asarray(cig, np.uint32))


def concat(batches):
    from coverm_amd.engine import RecordBatch
    cig = np.concatenate([b.cigar[int(b.cigar_off[0]):int(b.cigar_off[-1])] for b in batches]).astype(np.uint32)
    off, base = [np.zeros(1, np.uint32)], 0
    for b in batches:
        o = b.cigar_off.astype(np.int64) - int(b.cigar_off[0])
        off.append((o[1:] + base).astype(np.uint32))
        base += int(o[-1])
    c = lambda k: np.concatenate([getattr(b, k) for b in batches])      # noqa: E731
    return RecordBatch.from_arrays(c("tid"), c("pos"), c("flag"), c("mapq"), c("nm"), c("nm_kind"), c("l_seq"), np.concatenate(off), cig)


def take(b, order):
    """Records order[0..] of b as a new batch."""
    from coverm_amd.engine import RecordBatch
    order = np.asarray(order, np.int64)
    lens = (b.cigar_off[1:].astype(np.int64) - b.cigar_off[:-1])[order]
    off = np.concatenate([[0], np.cumsum(lens)])
    cig = np.concatenate([b.cigar[int(b.cigar_off[i]):int(b.cigar_off[i + 1])] for i in order]) if len(order) else np.zeros(0, np.uint32)
    return RecordBatch.from_arrays(b.tid[order], b.pos[order], b.flag[order], b.mapq[order], b.nm[order], b.nm_kind[order], b.l_seq[order], off, cig)
