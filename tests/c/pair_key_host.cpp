// csrc/pair_key_core.h on the CPU, as a program (tests/test_pair_key_core.py; also built with -fsanitize=address,undefined).
// Input, one case per line:
//   K  qh1  qh2  tid  mask          the key of a record and the slot its probe run starts at in a table of mask + 1 entries
//   Z  n                            the table's entries for a chunk of n records
// Output:
//   K: "K <k1> <k2t> <slot>"
//   Z: "Z <entries>"
#include <cstdio>

#include "../../coverm_amd/csrc/pair_key_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: pair_key_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        if (kind[0] == 'K') {
            unsigned long long qh1;
            unsigned qh2, mask;
            int tid;
            if (fscanf(fh, "%llu %u %d %u", &qh1, &qh2, &tid, &mask) != 4) return 3;
            const pkey::u64 k1 = pkey::key_k1(qh1), k2t = pkey::key_k2t(qh2, tid);
            printf("K %llu %llu %u\n", k1, k2t, pkey::table_slot(k1, k2t, mask));
        } else if (kind[0] == 'Z') {
            unsigned long long n;
            if (fscanf(fh, "%llu", &n) != 1) return 3;
            printf("Z %llu\n", pkey::table_size(n));
        } else return 3;
    }
    fclose(fh);
    return 0;
}
