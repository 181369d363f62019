"""SAM text rendered from a BamData, for the tests of the SAM text route: real QNAMEs, RNEXT / PNEXT / TLEN, a SEQ and QUAL of l_seq bytes,
NM and other tags.  What the tests expect is always oracle.bamio.read_sam of the text this writes, never the BamData it was written from."""
import numpy as np

from oracle.bamio import CIGAR_OPS, NM_UNSIGNED

_BASES = np.frombuffer(b"ACGT", np.uint8)


def render(b, seed=1, eol="\n", extra_header=("@HD\tVN:1.6\tSO:unknown", "@PG\tID:samtext\tPN:samtext")):
    """The SAM text of `b` as bytes."""
    rng = np.random.default_rng(seed)
    out = [extra_header[0]] if extra_header else []
    out += ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in zip(b.ref_names, b.ref_lens)]
    out += list(extra_header[1:]) if extra_header else []
    n = len(b.tid)
    mtid = np.asarray(b.mtid) if len(b.mtid) == n else np.full(n, -1)
    mpos = np.asarray(b.mpos) if len(b.mpos) == n else np.full(n, -1)
    tlen = np.asarray(b.tlen) if len(b.tlen) == n else np.zeros(n, np.int64)
    pool_seq = _BASES[rng.integers(0, 4, 1 << 16)].tobytes().decode()
    pool_qual = (rng.integers(2, 41, 1 << 16) + 33).astype(np.uint8).tobytes().decode()      # ('@' is among them: a QUAL may begin with it)
    at = rng.integers(0, 1 << 15, n)
    score = rng.integers(0, 300, n)
    for i in range(n):
        t, mt, ls = int(b.tid[i]), int(mtid[i]), int(b.l_seq[i])
        cig = "".join("%d%s" % (w >> 4, CIGAR_OPS[w & 15]) for w in b.cigar[b.cigar_off[i]:b.cigar_off[i + 1]]) or "*"
        rnext = "*" if mt < 0 else ("=" if mt == t else b.ref_names[mt])
        o = int(at[i])
        seq = (pool_seq[o:o + ls] if ls <= (1 << 15) else (pool_seq * (ls // (1 << 15) + 2))[o:o + ls]) if ls else "*"
        qual = (pool_qual[o:o + ls] if ls <= (1 << 15) else (pool_qual * (ls // (1 << 15) + 2))[o:o + ls]) if ls else "*"
        qn = b.qname[i].decode() if b.qname else "read%d" % i
        tags = ["AS:i:%d" % int(score[i])]
        if b.nm_kind[i] == NM_UNSIGNED:
            tags.append("NM:i:%d" % int(b.nm[i]))
        tags.append("MD:Z:%d" % max(ls, 1))
        out.append("\t".join([qn, str(int(b.flag[i])), b.ref_names[t] if t >= 0 else "*", str(int(b.pos[i]) + 1), str(int(b.mapq[i])), cig, rnext,
                              str(int(mpos[i]) + 1), str(int(tlen[i])), seq, qual] + tags))
    return (eol.join(out) + eol).encode()


def write(path, b, **kw):
    text = render(b, **kw)
    with open(path, "wb") as f:
        f.write(text)
    return text
