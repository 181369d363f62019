// csrc/gene_reads_core.h on the CPU, as a program (tests/test_gene_reads_core.py; also built with -fsanitize=address,undefined).
// Input, one case after the other:
//   S  inc_improper inc_supp inc_sec filter_single min_mapq min_aligned_length  min_percent_identity min_aligned_percent (f32 bit patterns, hex)
//      n_targets n n_iv want_identity
//      n lines:     tid pos flag mapq nm nm_kind l_seq n_cigar  word ...
//      n_iv lines:  tid start end
//   K  n  cs_0 len_0 ... : slices of the taken records of n contigs with genes, ascending
// Output:
//   S: "V <verdict key or -1> <sorted> <mapped_total>", one "C state primary mism ident-bits" per record, and (no verdict, sorted) one
//      "G n_reads mismatches sum_identity-bits contig_taken" per interval
//   K: "K <ck_slots>  base_0 ... base_{n-1}"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../coverm_amd/csrc/gene_reads_core.h"

static float f32_of(unsigned b) { float f; memcpy(&f, &b, 4); return f; }
static unsigned long long bits_of(double d) { unsigned long long b; memcpy(&b, &d, 8); return b; }

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: gene_reads_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        if (kind[0] == 'K') {
            unsigned n;
            if (fscanf(fh, "%u", &n) != 1) return 3;
            std::vector<unsigned> cs(n), len(n);
            for (unsigned k = 0; k < n; k++) if (fscanf(fh, "%u %u", &cs[k], &len[k]) != 2) return 3;
            const unsigned taken = n ? cs[n - 1] + len[n - 1] : 0u;
            printf("K %llu ", gnrc::ck_slots(taken, n));
            for (unsigned k = 0; k < n; k++) printf(" %llu", gnrc::ck_base(cs[k], k));
            printf("\n");
            continue;
        }
        gnrc::Filter f;
        unsigned pid, pal, nT, n, want;
        unsigned long long n_iv;
        if (fscanf(fh, "%u %u %u %u %u %u %x %x %u %u %llu %u", &f.include_improper_pairs, &f.include_supplementary, &f.include_secondary, &f.filter_single,
                   &f.min_mapq, &f.min_aligned_length, &pid, &pal, &nT, &n, &n_iv, &want) != 12) return 3;
        f.min_percent_identity = f32_of(pid); f.min_aligned_percent = f32_of(pal);
        std::vector<int32_t> tid(n), pos(n);
        std::vector<uint16_t> flag(n);
        std::vector<uint8_t> mapq(n), nmk(n);
        std::vector<gnrc::u32> nm(n), lseq(n), coff((size_t)n + 1, 0), cig;
        for (unsigned i = 0; i < n; i++) {
            unsigned fl, mq, k, nc;
            if (fscanf(fh, "%d %d %u %u %u %u %u %u", &tid[i], &pos[i], &fl, &mq, &nm[i], &k, &lseq[i], &nc) != 8) return 3;
            flag[i] = (uint16_t)fl; mapq[i] = (uint8_t)mq; nmk[i] = (uint8_t)k;
            for (unsigned c = 0; c < nc; c++) { unsigned w; if (fscanf(fh, "%u", &w) != 1) return 3; cig.push_back(w); }
            coff[i + 1] = (gnrc::u32)cig.size();
        }
        std::vector<gnrc::Interval> iv(n_iv);
        for (auto &v : iv) { if (fscanf(fh, "%u %llu %llu", &v.tid, &v.start, &v.end) != 3) return 3; v.pad = 0; }
        // exactly the sizes the header promises to stay inside: the sanitized build sees any step outside them
        std::vector<int32_t> t_tid(n), t_pos(n);
        std::vector<double> t_ident(n), p_before(n);
        std::vector<gnrc::u64> pprim((size_t)n + 1), pmism((size_t)n + 1);
        std::vector<gnrc::Aggregate> out(n_iv);
        gnrc::u64 mapped = 0;
        int sorted = 0;
        const gnrc::u64 v = gnrc::aggregates_cpu(f, nT, n, tid.data(), pos.data(), flag.data(), mapq.data(), nm.data(), nmk.data(), lseq.data(), coff.data(), cig.data(),
                                                 iv.data(), n_iv, (int)want, t_tid.data(), t_pos.data(), t_ident.data(), p_before.data(), pprim.data(), pmism.data(),
                                                 out.data(), &mapped, &sorted);
        if (v == gnrc::NO_VERDICT) printf("V -1 %d %llu\n", sorted, mapped); else printf("V %llu %d %llu\n", v, sorted, mapped);
        for (unsigned i = 0; i < n; i++) {
            gnrc::u64 aligned = 0, indels = 0;
            for (gnrc::u32 c = coff[i]; c < coff[i + 1]; c++) gnrc::cigar_add(cig[c], aligned, indels);
            const gnrc::Class c = gnrc::classify(f, flag[i], mapq[i], nmk[i], nm[i], lseq[i], aligned, indels);
            printf("C %u %u %llu %llx\n", c.state, c.primary, c.mism, bits_of(c.ident));
        }
        if (v == gnrc::NO_VERDICT && sorted)
            for (const auto &o : out) printf("G %llu %llu %llx %llu\n", o.n_reads, o.mismatches, bits_of(o.sum_identity), o.contig_taken);
    }
    fclose(fh);
    return 0;
}
