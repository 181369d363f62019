// csrc/sep_entry_core.h on the CPU, as a program (tests/test_sep_entry_core.py; also built with -fsanitize=address,undefined).
// Input, one case per line:   n  gid[0] .. gid[n-1]  obs[0] .. obs[n-1]
// Output, one line per case:  n_entries ; row[0 .. n_entries] ; tids[0 .. row[n_entries]) ; first_tid[] ; entry_gid[]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../coverm_amd/csrc/sep_entry_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: sep_entry_host <cases>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    unsigned n;
    std::vector<int32_t> gid, egid;
    std::vector<uint8_t> obs;
    std::vector<sepc::u32> blk, prev1, next, row, tids, first;
    while (fscanf(f, "%u", &n) == 1) {
        gid.resize(n); obs.resize(n);
        for (unsigned t = 0; t < n; t++) if (fscanf(f, "%d", &gid[t]) != 1) return 3;
        for (unsigned t = 0; t < n; t++) { unsigned o; if (fscanf(f, "%u", &o) != 1) return 3; obs[t] = (uint8_t)o; }
        // exactly the sizes the header promises to stay inside: the sanitized build sees any step outside them
        blk.assign(n, 0); prev1.assign(n, 0); next.assign(n, 0); row.assign((size_t)n + 1, 0); tids.assign(n, 0); first.assign(n, 0); egid.assign(n, 0);
        const sepc::u32 ne = sepc::entries_cpu(gid.data(), obs.data(), n, blk.data(), prev1.data(), next.data(), row.data(), tids.data(), first.data(), egid.data());
        if (ne > n || row[ne] > n) return 4;
        printf("%u ;", ne);
        for (unsigned e = 0; e <= ne; e++) printf(" %u", row[e]);
        printf(" ;");
        for (unsigned i = 0; i < row[ne]; i++) printf(" %u", tids[i]);
        printf(" ;");
        for (unsigned e = 0; e < ne; e++) printf(" %u", first[e]);
        printf(" ;");
        for (unsigned e = 0; e < ne; e++) printf(" %d", egid[e]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
