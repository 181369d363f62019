// csrc/bam_record_core.h on the CPU: the record test, the NM scan and the CG:B,I lookup, each with the byte-walking policy (Serial: what one
// lane does) and with the wave's string walk lane by lane (Lanes64: 1024-byte steps of 16 bytes per lane through lane_nul_mask, the
// function the kernels call).  As a shared library for tests/test_bam_record_core.py, which compares both with a Python restatement; as a
// program (BAMREC_HOST_MAIN, or simply run: main is always there) it builds its own records and walks the same kinds of cases, for a run
// under -fsanitize=address,undefined.
// Buffers handed in are 4-byte aligned with at least 16 readable bytes behind N, as the device's window buffers are.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../coverm_amd/csrc/bam_record_core.h"

using bamrec::u32;
using bamrec::u64;

namespace {
bamrec::Stream stream_of(const uint8_t *u, u64 N, int n_ref, const u32 *ref_len, u64 walk_cap) { return bamrec::Stream{u, N, n_ref, ref_len, walk_cap}; }
}

extern "C" {
u32 bamrec_long_cigar_words() { return bamrec::LONG_CIGAR_WORDS; }
u32 bamrec_long_aux_bytes() { return bamrec::LONG_AUX_BYTES; }
int bamrec_is_long(u32 words, u64 aux_bytes) { return bamrec::is_long(words, aux_bytes) ? 1 : 0; }
// end offset of the record that can start at o, or 0
u64 bamrec_plausible(const uint8_t *u, u64 N, int n_ref, const u32 *ref_len, u64 walk_cap, int wave, u64 o) {
    const bamrec::Stream S = stream_of(u, N, n_ref, ref_len, walk_cap);
    return wave ? bamrec::plausible_record(bamrec::Lanes64{}, S, o) : bamrec::plausible_record(bamrec::Serial{}, S, o);
}
// out[o] = 1 where a chain starts: the per-lane filter first, as k_bam_find does, then the chain
void bamrec_chain_starts(const uint8_t *u, u64 N, int n_ref, const u32 *ref_len, u64 walk_cap, int wave, uint8_t *out) {
    const bamrec::Stream S = stream_of(u, N, n_ref, ref_len, walk_cap);
    for (u64 o = 0; o < N; o++) {
        u64 aux = 0;
        out[o] = 0;
        if (!bamrec::fixed_fields(S, o, aux)) continue;
        out[o] = (wave ? bamrec::chain_start(bamrec::Lanes64{}, S, o) : bamrec::chain_start(bamrec::Serial{}, S, o)) ? 1 : 0;
    }
}
u32 bamrec_scan_nm(const uint8_t *u, u64 p, u64 end, int wave, u32 *nm) {
    return wave ? bamrec::scan_nm(bamrec::Lanes64{}, u, p, end, *nm) : bamrec::scan_nm(bamrec::Serial{}, u, p, end, *nm);
}
u64 bamrec_cg_cigar(const uint8_t *u, u64 r, u64 end, int wave, u32 *cnt) {
    return wave ? bamrec::cg_cigar(bamrec::Lanes64{}, u, r, end, *cnt) : bamrec::cg_cigar(bamrec::Serial{}, u, r, end, *cnt);
}
}

// ------------------------------------------------------------------------------------------------ the program
namespace {
typedef std::string Bytes;
void put32(Bytes &b, u32 v) { for (int i = 0; i < 4; i++) b.push_back((char)(v >> (8 * i))); }
void put16(Bytes &b, u32 v) { b.push_back((char)v); b.push_back((char)(v >> 8)); }
Bytes tagZ(const char *n, size_t len, char fill = 'x') { Bytes b(n, 2); b.push_back('Z'); b.append(len, fill); b.push_back('\0'); return b; }
Bytes tagS(const char *n, char ty, u32 v) {
    Bytes b(n, 2); b.push_back(ty);
    const u32 sz = bamrec::scalar_size((uint8_t)ty);
    for (u32 i = 0; i < sz; i++) b.push_back((char)(v >> (8 * i)));
    return b;
}
Bytes tagB(const char *n, char st, u32 cnt, u32 fill = 0) {
    Bytes b(n, 2); b.push_back('B'); b.push_back(st); put32(b, cnt);
    b.append((size_t)cnt * bamrec::array_elem_size((uint8_t)st), (char)fill);
    return b;
}
Bytes record(int tid, int pos, const std::vector<u32> &cigar, u32 l_seq, const Bytes &aux, const Bytes &name = "q") {
    Bytes b;
    put32(b, (u32)tid); put32(b, (u32)pos); b.push_back((char)(name.size() + 1)); b.push_back(30); put16(b, 4680); put16(b, (u32)cigar.size()); put16(b, 0);
    put32(b, l_seq); put32(b, (u32)-1); put32(b, (u32)-1); put32(b, 0);
    b += name; b.push_back('\0');
    for (u32 c : cigar) put32(b, c);
    b.append((l_seq + 1) / 2, '\x11'); b.append(l_seq, '\xff');
    b += aux;
    Bytes r; put32(r, (u32)b.size());
    return r + b;
}
struct Buf {      // aligned, padded copy
    std::vector<u32> w; u64 N;
    explicit Buf(const Bytes &b) : w((b.size() + 16 + 3) / 4 + 1, 0u), N(b.size()) { memcpy(w.data(), b.data(), b.size()); }
    const uint8_t *u() const { return reinterpret_cast<const uint8_t *>(w.data()); }
};
const u32 REF_LEN[2] = {2000000u, 50000u};
int cases = 0, bad = 0;
void expect(bool ok, const char *what, long long a = 0) { cases++; if (!ok) { bad++; fprintf(stderr, "FAIL %s (%lld)\n", what, a); } }
// one record alone in a stream: plausible (both policies agree) or not
bool plausible_alone(const Bytes &rec, u64 cap = 1ull << 24) {
    Buf B(rec);
    const u64 a = bamrec_plausible(B.u(), B.N, 2, REF_LEN, cap, 0, 0), b = bamrec_plausible(B.u(), B.N, 2, REF_LEN, cap, 1, 0);
    expect(a == b, "serial and wave walks agree", (long long)rec.size());
    return a == B.N;
}
Bytes with_aux(const Bytes &aux) { return record(0, 100, {100u << 4}, 100, aux); }
u32 nm_of(const Bytes &aux, u32 &nm) {
    Buf B(aux);
    u32 n0 = 0, n1 = 0;
    const u32 k0 = bamrec_scan_nm(B.u(), 0, B.N, 0, &n0), k1 = bamrec_scan_nm(B.u(), 0, B.N, 1, &n1);
    expect(k0 == k1 && n0 == n1, "NM: serial and wave scans agree");
    nm = n0;
    return k0;
}
}  // namespace

int main() {
    // a stream of records with mixed tags: exactly the true starts head chains
    {
        Bytes s; std::vector<u64> starts;
        u32 x = 12345;
        while (s.size() < 200000) {
            x = x * 1664525u + 1013904223u;
            Bytes aux = tagS("NM", 'C', x & 7u);
            if (x & 16u) aux += tagZ("MD", (x >> 8) % 3000u, '7');
            if (x & 32u) aux += tagB("ML", 'C', (x >> 10) % 5000u, (x >> 3) & 0xffu);
            if (x & 64u) aux += tagS("AS", 'i', x) + tagS("XA", 'A', 'k') + tagS("XS", 's', 7) + tagS("XF", 'f', 0x3f800000u);
            if (x & 128u) aux += tagZ("SA", (x >> 12) % 200u, ',') + tagB("XI", 'I', (x >> 20) % 40u) + tagB("XH", 's', 3) + Bytes("XQH41\0", 6);
            starts.push_back(s.size());
            const u32 l_seq = 30 + (x >> 24);
            s += record((int)((x >> 5) & 1u), (int)(x % 40000u), {l_seq << 4}, l_seq, aux, "read" + std::to_string(x & 1023u));
        }
        Buf B(s);
        std::vector<uint8_t> a(B.N), b(B.N);
        bamrec_chain_starts(B.u(), B.N, 2, REF_LEN, 1ull << 24, 0, a.data());
        bamrec_chain_starts(B.u(), B.N, 2, REF_LEN, 1ull << 24, 1, b.data());
        size_t at = 0; u64 wrong = 0;
        for (u64 o = 0; o < B.N; o++) {
            const bool is_start = at < starts.size() && starts[at] == o;
            if (is_start) at++;
            if ((a[o] != 0) != is_start || a[o] != b[o]) wrong++;
        }
        expect(wrong == 0, "exactly the true starts have chains, both walks", (long long)wrong);
    }
    for (size_t len : {0u, 1u, 4095u, 4096u, 4097u, 65535u, 65536u, 200000u})
        expect(plausible_alone(with_aux(tagS("NM", 'C', 1) + tagZ("MM", len))), "Z string length", (long long)len);
    for (int n : {1, 31, 32, 33, 64}) {
        Bytes aux;
        for (int i = 0; i < n; i++) { const char nm[2] = {'X', (char)('0' + i % 10)}; aux += (i % 3 == 0) ? tagZ(nm, (size_t)i) : tagS(nm, "cCsSiIfA"[i % 8], (u32)i); }
        expect(plausible_alone(with_aux(aux)), "tag count", n);
    }
    {   // a malformed 33rd tag (unknown type with the right number of bytes)
        Bytes aux;
        for (int i = 0; i < 32; i++) aux += tagS("XX", 'i', (u32)i);
        expect(!plausible_alone(with_aux(aux + Bytes("YYq\1\2\3\4", 7))), "malformed 33rd tag");
    }
    for (const char *ty = "AcCsSiIf"; *ty; ty++) expect(plausible_alone(with_aux(tagS("XT", *ty, 65))), "scalar type", *ty);
    expect(plausible_alone(with_aux(tagZ("XZ", 9) + Bytes("XHH1F\0", 6))), "Z and H");
    for (const char *st = "cCsSiIf"; *st; st++) expect(plausible_alone(with_aux(tagB("XB", *st, 11, 3))), "B subtype", *st);
    expect(!plausible_alone(with_aux(Bytes("XBBd\1\0\0\0\0\0\0\0", 12))), "B of an unknown subtype");
    {   // a count that runs past the end, a tag cut by the end, an area one byte short or long
        Bytes b = tagB("XB", 'I', 4); b[4] = 5;
        expect(!plausible_alone(with_aux(b)), "B count past the record end");
        expect(!plausible_alone(with_aux(tagS("XI", 'i', 1).substr(0, 6))), "scalar cut by the end");
        expect(!plausible_alone(with_aux(Bytes("XI", 2))), "two bytes of a tag");
        expect(!plausible_alone(with_aux(tagZ("XZ", 50).substr(0, 53))), "string without its NUL");
        Bytes r = with_aux(tagS("NM", 'C', 1) + tagZ("XZ", 50));
        Bytes early = r; early[0] = (char)(early[0] - 1); early.pop_back();
        expect(!plausible_alone(early), "area ends one byte early");
        Bytes late = r; late[0] = (char)(late[0] + 1); late.push_back('\0');
        expect(!plausible_alone(late), "area ends one byte late");
    }
    {   // block_size above the walk bound
        const Bytes r = with_aux(tagZ("MM", 5000));
        expect(plausible_alone(r, r.size() - 4), "block_size at the bound");
        expect(!plausible_alone(r, r.size() - 5), "block_size above the bound");
    }
    {   // NM first, last, 36th; its types; absent
        u32 nm = 0;
        Bytes many;
        for (int i = 0; i < 35; i++) many += (i % 4 == 0) ? tagZ("XZ", (size_t)(i * 37)) : (i % 4 == 1) ? tagB("XB", 'S', (u32)i) : tagS("XS", 'i', (u32)i);
        expect(nm_of(tagS("NM", 'C', 200) + many, nm) == 1 && nm == 200, "NM:C first");
        expect(nm_of(many + tagS("NM", 'S', 60000), nm) == 1 && nm == 60000, "NM:S 36th and last");
        expect(nm_of(many + tagS("NM", 'I', 3000000000u) + many, nm) == 1 && nm == 3000000000u, "NM:I 36th of 71");
        expect(nm_of(many + tagS("NM", 'i', 5), nm) == 2, "NM:i");
        expect(nm_of(many + tagZ("NM", 3), nm) == 2, "NM:Z");
        expect(nm_of(many + tagB("NM", 'C', 3), nm) == 2, "NM:B");
        expect(nm_of(many, nm) == 0, "no NM");
        expect(nm_of(Bytes(), nm) == 0, "no tags");
        expect(nm_of(Bytes("XXq\1", 4) + tagS("NM", 'C', 1), nm) == 0, "NM behind a tag that does not parse");
    }
    {   // CG:B,I behind a long Z
        const u32 n_ops = 70001, l_seq = 500;
        Bytes cg = tagB("CG", 'I', n_ops, 0x20);
        const Bytes aux = tagS("NM", 'C', 5) + tagZ("MM", 8000) + cg;
        const Bytes r = record(0, 100, {(l_seq << 4) | 4u, (900u << 4) | 3u}, l_seq, aux);
        Buf B(r);
        u32 c0 = 0, c1 = 0;
        const u64 a = bamrec_cg_cigar(B.u(), 0, B.N, 0, &c0), b = bamrec_cg_cigar(B.u(), 0, B.N, 1, &c1);
        expect(a == b && c0 == n_ops && c1 == n_ops && a == B.N - 4ull * n_ops, "CG:B,I behind a long Z");
        const Bytes plain = record(0, 100, {(l_seq << 4) | 4u, (900u << 4) | 3u}, l_seq, tagS("NM", 'C', 5) + tagZ("MM", 8000));
        Buf P(plain);
        expect(bamrec_cg_cigar(P.u(), 0, P.N, 1, &c1) == bamrec::NONE, "no CG");
        expect(bamrec_is_long(64, 1024) == 0 && bamrec_is_long(65, 0) == 1 && bamrec_is_long(0, 1025) == 1, "long-record thresholds");
    }
    printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
