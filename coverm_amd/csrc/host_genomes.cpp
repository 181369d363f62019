// host_genomes.cpp — genomes defined by FASTA files (`coverm genome -f / -d -x / --genome-fasta-list`), host C++.
//
// read_genome_fasta_files (src/genome_parsing.rs:10-70) + GenomesAndContigs::insert (src/genomes_and_contigs.rs:25-40):
// one genome per file, named by the file stem of its path once a `.gz` / `.bz` / `.xz` is cut off; its contigs are the
// record ids of the file, cut at the first space unless full names are asked for; a contig in two records — of two files
// or of one — is an error.  The directory and list forms of bird_tool_utils' parse_list_of_genome_fasta_files resolve to a
// list of paths first (covh_genome_fasta_paths).
//
// Only the header lines matter.  `>` cannot occur in sequence lines, so a record starts at every `>` that follows a newline
// (or starts the file): the scan is memchr over the bytes and never looks at a base.  Files are read in parallel (bounded by
// the caller's thread count); a large plain file is cut into fixed ranges that are scanned in parallel as well.  The table is
// then built serially in file order, so genome order, contig order and the first error do not depend on the thread count.
// Input format by magic bytes, as needletail detects it: plain text and gzip (multi-member and BGZF included, through zlib);
// bzip2, xz and zstd are refused with an error that names the format.  Nothing here touches the GPU.
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/coverm_host.h"

struct covh_path_list {
    std::vector<std::string> paths;
};

struct covh_genome_set {
    std::vector<std::string> genomes;
    std::string blob;                      // contig names, each followed by a NUL
    std::vector<uint64_t> name_off;        // n_contigs + 1 (offsets include the NULs)
    std::vector<int32_t> genome_of;        // per contig, in file order
    std::vector<uint32_t> table;           // open addressing: contig index + 1, 0 = empty
    uint64_t mask = 0;
    const char *name(size_t i) const { return blob.data() + name_off[i]; }
    size_t len(size_t i) const { return name_off[i + 1] - name_off[i] - 1; }
};

namespace {

constexpr uint64_t kRange = 32ull << 20;          // a plain file above 2 ranges is scanned as ranges of this size
constexpr size_t kBuf = 1u << 20;

void set_err(char *err, size_t errcap, const std::string &m) {
    if (err && errcap) snprintf(err, errcap, "%s", m.c_str());
}

inline uint64_t hash_name(const char *p, size_t n) {   // FNV-1a, 64 bit
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= (uint8_t)p[i]; h *= 1099511628211ull; }
    return h ^ (h >> 29);
}

// genome_parsing.rs:22-40: the whole path cut at its last ".gz", else ".bz", else ".xz"; then Rust's Path::file_stem
bool genome_name_of(const std::string &path, std::string &out) {
    std::string p = path;
    size_t i;
    if ((i = p.rfind(".gz")) != std::string::npos) p.resize(i);
    else if ((i = p.rfind(".bz")) != std::string::npos) p.resize(i);
    else if ((i = p.rfind(".xz")) != std::string::npos) p.resize(i);
    for (;;) {   // Path::file_name skips trailing separators and "." components
        while (p.size() > 1 && p.back() == '/') p.pop_back();
        if (p.size() >= 2 && p.compare(p.size() - 2, 2, "/.") == 0) { p.resize(p.size() - 2); continue; }
        break;
    }
    const size_t sl = p.rfind('/');
    const std::string name = sl == std::string::npos ? p : p.substr(sl + 1);
    if (name.empty() || name == "." || name == "..") return false;
    const size_t d = name.rfind('.');
    out = (d == std::string::npos || d == 0) ? name : name.substr(0, d);   // ".hidden" keeps its dot
    return true;
}

// What one file (or one range of a large plain file) yields: its contig names in order, and the error that ended it.
struct Part {
    std::string names;            // each followed by a NUL
    std::vector<uint64_t> ends;   // end of each name in `names` (before its NUL)
    std::string err;
};

// Record starts in a byte stream: a '>' at the start of the stream or after '\n'.  A header line is kept up to its '\n'
// (a '\r' before it dropped) and cut at its first space unless full names are kept.
struct Scanner {
    Part &out;
    const std::string &path;
    bool full;
    bool first;          // the next byte is the first of the file: it must be '>'
    bool nl = true;      // the byte before the next one was '\n'
    bool in_hdr = false;
    std::string hdr;
    Scanner(Part &o, const std::string &p, bool f, bool at_file_start) : out(o), path(p), full(f), first(at_file_start) {}

    void finish_header() {
        if (!hdr.empty() && hdr.back() == '\r') hdr.pop_back();
        size_t n = hdr.size();
        if (!full) { const size_t sp = hdr.find(' '); if (sp != std::string::npos) n = sp; }
        out.names.append(hdr.data(), n);
        out.ends.push_back(out.names.size());
        out.names.push_back('\0');
        in_hdr = false;
        hdr.clear();
    }
    // Bytes [p, p + n), the first at absolute offset `at`; '>' at offsets >= stop do not start records here.  Returns true when
    // the scan is over (an error, or past `stop` with no header open).
    bool feed(const char *p, size_t n, uint64_t at, uint64_t stop) {
        if (!n) return false;
        if (first) {
            first = false;
            if (p[0] == '@') { out.err = "File \"" + path + "\" is not a fasta file, but a Fastq"; return true; }
            if (p[0] != '>') { out.err = "File \"" + path + "\" is not a fasta file: it does not start with '>'"; return true; }
        }
        const bool last_nl = p[n - 1] == '\n';
        size_t i = 0;
        while (i < n) {
            if (in_hdr) {
                const char *e = (const char *)memchr(p + i, '\n', n - i);
                if (!e) { hdr.append(p + i, n - i); break; }
                hdr.append(p + i, (size_t)(e - (p + i)));
                finish_header();
                i = (size_t)(e - p) + 1;
                continue;
            }
            if (at + i >= stop) return true;
            const size_t lim = (size_t)std::min<uint64_t>(n, stop - at);
            const char *q = (const char *)memchr(p + i, '>', lim - i);
            if (!q) { i = lim; continue; }
            const size_t j = (size_t)(q - p);
            if (j == 0 ? nl : p[j - 1] == '\n') in_hdr = true;
            i = j + 1;
        }
        nl = last_nl;
        return false;
    }
    void end_of_stream() { if (in_hdr) finish_header(); }
};

enum Kind { PLAIN, GZIP, BZIP2, XZ, ZSTD };

struct File {
    std::string path;
    uint64_t size = 0;
    std::string err_open;          // before the genome is established: unreadable, empty, unsupported compression
    std::vector<Part> parts;       // one, or one per range of a large plain file
};

bool pread_all(int fd, char *buf, size_t n, uint64_t off, size_t &got) {
    got = 0;
    while (got < n) {
        const ssize_t r = pread(fd, buf + got, n - got, (off_t)(off + got));
        if (r < 0) { if (errno == EINTR) continue; return false; }
        if (r == 0) break;
        got += (size_t)r;
    }
    return true;
}

// Plain bytes [start, stop) of a file (a header that begins before `stop` is read to its end).
void scan_plain(int fd, const std::string &path, bool full, uint64_t start, uint64_t stop, uint64_t size, std::vector<char> &buf, Part &part) {
    Scanner sc(part, path, full, start == 0);
    if (start > 0) {
        char b = 0; size_t got = 0;
        if (!pread_all(fd, &b, 1, start - 1, got) || got != 1) { part.err = "Failed to parse record in fasta file \"" + path + "\": read error"; return; }
        sc.nl = b == '\n';
    }
    uint64_t off = start;
    while (off < size) {
        size_t got = 0;
        if (!pread_all(fd, buf.data(), (size_t)std::min<uint64_t>(kBuf, size - off), off, got)) {
            part.err = "Failed to parse record in fasta file \"" + path + "\": " + strerror(errno);
            return;
        }
        if (got == 0) break;       // the file shrank
        if (sc.feed(buf.data(), got, off, stop)) break;
        off += got;
    }
    if (part.err.empty()) sc.end_of_stream();
}

// A gzip stream (members one after another: plain multi-member files and BGZF alike).  A stream that ends before its first
// decompressed byte is an open error; errors after that end the file's part.
void scan_gzip(int fd, File &f, bool full, std::vector<char> &in, std::vector<char> &outbuf) {
    f.parts.resize(1);
    Part &part = f.parts[0];
    Scanner sc(part, f.path, full, true);
    z_stream zs; memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 16) != Z_OK) { f.err_open = "Unable to read fasta file " + f.path + ": zlib initialisation failed"; return; }
    struct End { z_stream &z; ~End() { inflateEnd(&z); } } end{zs};
    uint64_t produced = 0, off = 0;
    bool member_open = false, eof = false;
    std::string bad;
    while (bad.empty()) {
        if (zs.avail_in == 0) {
            if (eof) break;
            size_t got = 0;
            if (!pread_all(fd, in.data(), in.size(), off, got)) { bad = strerror(errno); break; }
            if (got == 0) { eof = true; break; }
            off += got;
            zs.next_in = (Bytef *)in.data(); zs.avail_in = (uInt)got;
        }
        member_open = true;
        zs.next_out = (Bytef *)outbuf.data(); zs.avail_out = (uInt)outbuf.size();
        const int rc = inflate(&zs, Z_NO_FLUSH);
        const size_t n = outbuf.size() - zs.avail_out;
        if (n && sc.feed(outbuf.data(), n, produced, ~0ull)) return;
        produced += n;
        if (rc == Z_STREAM_END) { member_open = false; inflateReset(&zs); continue; }
        if (rc == Z_BUF_ERROR && n == 0 && zs.avail_in != 0) { bad = "gzip stream error"; break; }
        if (rc != Z_OK && rc != Z_BUF_ERROR) { bad = zs.msg ? zs.msg : "corrupt gzip stream"; break; }
    }
    if (bad.empty() && member_open) bad = "the gzip stream is truncated";
    if (produced == 0) {
        f.err_open = "Unable to read fasta file " + f.path + (bad.empty() ? std::string(": the file is empty") : ": " + bad);
        return;
    }
    if (!bad.empty()) { part.err = "Failed to parse record in fasta file \"" + f.path + "\": " + bad; return; }
    sc.end_of_stream();
}

// Opens a file, learns its format and either scans it whole or leaves its ranges for the second pass.
void open_and_scan(File &f, bool full, std::vector<char> &in, std::vector<char> &outbuf, std::vector<char> &buf) {
    const int fd = open(f.path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) { f.err_open = "Unable to read fasta file " + f.path + ": " + strerror(errno); return; }
    struct Close { int fd; ~Close() { close(fd); } } closer{fd};
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        f.err_open = "Unable to read fasta file " + f.path + ": not a regular file";
        return;
    }
    f.size = (uint64_t)st.st_size;
    unsigned char m[6] = {0, 0, 0, 0, 0, 0};
    size_t got = 0;
    if (!pread_all(fd, (char *)m, sizeof m, 0, got)) { f.err_open = "Unable to read fasta file " + f.path + ": " + strerror(errno); return; }
    if (got == 0) { f.err_open = "Unable to read fasta file " + f.path + ": the file is empty"; return; }
    Kind k = PLAIN;
    if (got >= 2 && m[0] == 0x1f && m[1] == 0x8b) k = GZIP;
    else if (got >= 3 && m[0] == 'B' && m[1] == 'Z' && m[2] == 'h') k = BZIP2;
    else if (got >= 6 && m[0] == 0xfd && !memcmp(m + 1, "7zXZ", 4) && m[5] == 0) k = XZ;
    else if (got >= 4 && m[0] == 0x28 && m[1] == 0xb5 && m[2] == 0x2f && m[3] == 0xfd) k = ZSTD;
    if (k == BZIP2 || k == XZ || k == ZSTD) {
        f.err_open = "Unable to read fasta file " + f.path + ": " + (k == BZIP2 ? "bzip2" : k == XZ ? "xz" : "zstd") +
                     "-compressed input is not supported (plain text and gzip are)";
        return;
    }
    if (k == GZIP) { scan_gzip(fd, f, full, in, outbuf); return; }
    const uint64_t nr = f.size > 2 * kRange ? (f.size + kRange - 1) / kRange : 1;
    f.parts.resize(nr);
    if (nr == 1) scan_plain(fd, f.path, full, 0, f.size, f.size, buf, f.parts[0]);
}

// Runs fn(i) for i in [0, n) on up to `threads` threads.
template <class Fn>
void parallel_for(size_t n, int threads, Fn fn) {
    const size_t nt = std::min<size_t>(n, (size_t)std::max(1, threads));
    if (nt <= 1) { for (size_t i = 0; i < n; i++) fn(i, 0); return; }
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++)
        th.emplace_back([&, t] { for (size_t i; (i = next.fetch_add(1)) < n;) fn(i, t); });
    for (auto &x : th) x.join();
}

}  // namespace

extern "C" {

covh_path_list *covh_genome_fasta_paths(const char *directory, const char *extension, const char *list_file, char *err, size_t errcap) {
    if ((directory != nullptr) == (list_file != nullptr)) { set_err(err, errcap, "give exactly one of a genome FASTA directory and a genome FASTA list"); return nullptr; }
    auto *l = new covh_path_list();
    if (directory) {
        std::string ext = extension ? extension : "fna";
        if (!ext.empty() && ext[0] == '.') ext.erase(0, 1);         // "-x .fna" == "-x fna"
        const std::string suffix = "." + ext;
        std::string dir = directory;
        while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
        DIR *d = opendir(dir.c_str());
        if (!d) { set_err(err, errcap, "Unable to read genome FASTA directory " + dir + ": " + strerror(errno)); delete l; return nullptr; }
        std::vector<std::string> names;
        while (struct dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() < suffix.size() || n.compare(n.size() - suffix.size(), suffix.size(), suffix) != 0) continue;
            const std::string p = (dir == "/" ? std::string() : dir) + "/" + n;
            struct stat st;
            if (stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode)) names.push_back(p);   // symlinks followed
        }
        closedir(d);
        std::sort(names.begin(), names.end());     // bytewise: directory order is unspecified
        l->paths = std::move(names);
        if (l->paths.empty()) {
            set_err(err, errcap, "No genome FASTA files with extension ." + ext + " were found in directory " + dir);
            delete l;
            return nullptr;
        }
    } else {
        FILE *fh = fopen(list_file, "rb");
        if (!fh) { set_err(err, errcap, std::string("Unable to read genome FASTA list ") + list_file + ": " + strerror(errno)); delete l; return nullptr; }
        std::string all;
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fh)) > 0) all.append(buf, n);
        fclose(fh);
        for (size_t p = 0; p < all.size();) {
            size_t q = all.find('\n', p);
            if (q == std::string::npos) q = all.size();
            std::string line = all.substr(p, q - p);
            p = q + 1;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty()) l->paths.push_back(line);
        }
        if (l->paths.empty()) {
            set_err(err, errcap, std::string("No genome FASTA files were listed in ") + list_file);
            delete l;
            return nullptr;
        }
    }
    return l;
}

size_t covh_path_list_count(const covh_path_list *l) { return l ? l->paths.size() : 0; }
const char *covh_path_list_get(const covh_path_list *l, size_t i) { return l && i < l->paths.size() ? l->paths[i].c_str() : nullptr; }
void covh_path_list_free(covh_path_list *l) { delete l; }

covh_genome_set *covh_genome_set_from_fasta(const char *const *paths, size_t n, int use_full_contig_names, int threads, char *err, size_t errcap) {
    const bool full = use_full_contig_names != 0;
    std::vector<File> files(n);
    for (size_t i = 0; i < n; i++) files[i].path = paths[i] ? paths[i] : "";
    threads = std::max(1, std::min(threads, 1024));
    struct Bufs { std::vector<char> in, out, buf; };
    std::vector<Bufs> bufs((size_t)threads);
    auto bufs_of = [&](size_t t) -> Bufs & {
        Bufs &b = bufs[t];
        if (b.buf.empty()) { b.in.resize(kBuf); b.out.resize(kBuf); b.buf.resize(kBuf); }
        return b;
    };
    // pass 1: every file opened, classified; small plain and every gzip file scanned whole
    parallel_for(n, threads, [&](size_t i, size_t t) { Bufs &b = bufs_of(t); open_and_scan(files[i], full, b.in, b.out, b.buf); });
    // pass 2: the ranges of large plain files
    std::vector<std::pair<size_t, size_t>> ranges;
    for (size_t i = 0; i < n; i++)
        if (files[i].err_open.empty() && files[i].parts.size() > 1)
            for (size_t r = 0; r < files[i].parts.size(); r++) ranges.emplace_back(i, r);
    parallel_for(ranges.size(), threads, [&](size_t k, size_t t) {
        File &f = files[ranges[k].first];
        const size_t r = ranges[k].second;
        Part &part = f.parts[r];
        const int fd = open(f.path.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd < 0) { part.err = "Failed to parse record in fasta file \"" + f.path + "\": " + strerror(errno); return; }
        const uint64_t s = (uint64_t)r * kRange, e = std::min(f.size, s + kRange);
        scan_plain(fd, f.path, full, s, e, f.size, bufs_of(t).buf, part);
        close(fd);
    });

    // the table, serially in file order: genome order, contig order and the first error are those of a one-file-at-a-time read
    auto *gs = new covh_genome_set();
    size_t total = 0, bytes = 0;
    for (auto &f : files)
        for (auto &p : f.parts) { total += p.ends.size(); bytes += p.names.size(); }
    gs->blob.reserve(bytes);
    gs->name_off.reserve(total + 1);
    gs->genome_of.reserve(total);
    uint64_t cap = 16;
    while (cap < 2 * (uint64_t)total) cap <<= 1;
    gs->table.assign(cap, 0);
    gs->mask = cap - 1;
    gs->name_off.push_back(0);
    std::unordered_map<std::string, int32_t> genome_index;
    genome_index.reserve(n);
    auto fail = [&](const std::string &m) { set_err(err, errcap, m); delete gs; return nullptr; };
    for (auto &f : files) {
        if (!f.err_open.empty()) return fail(f.err_open);
        std::string g;
        if (!genome_name_of(f.path, g)) return fail("Problem while determining file stem of " + f.path);
        if (!genome_index.emplace(g, (int32_t)gs->genomes.size()).second) return fail("The genome name " + g + " was derived from >1 file");
        const int32_t gi = (int32_t)gs->genomes.size();
        gs->genomes.push_back(g);
        for (auto &p : f.parts) {
            uint64_t b = 0;
            for (uint64_t e : p.ends) {
                const char *nm = p.names.data() + b;
                const size_t len = (size_t)(e - b);
                b = e + 1;
                uint64_t h = hash_name(nm, len) & gs->mask;
                for (;; h = (h + 1) & gs->mask) {
                    const uint32_t slot = gs->table[h];
                    if (!slot) break;
                    const size_t c = slot - 1;
                    if (gs->len(c) == len && !memcmp(gs->name(c), nm, len))
                        return fail("The contig '" + std::string(nm, len) + "' has been assigned to multiple genomes, at least '" +
                                    gs->genomes[(size_t)gs->genome_of[c]] + "' and '" + g + "'");
                }
                const size_t c = gs->genome_of.size();
                gs->table[h] = (uint32_t)(c + 1);
                gs->blob.append(nm, len + 1);
                gs->name_off.push_back(gs->blob.size());
                gs->genome_of.push_back(gi);
            }
            if (!p.err.empty()) return fail(p.err);
            std::string().swap(p.names);
        }
    }
    return gs;
}

size_t covh_genome_set_n_genomes(const covh_genome_set *s) { return s ? s->genomes.size() : 0; }
const char *covh_genome_set_genome_name(const covh_genome_set *s, size_t g) { return s && g < s->genomes.size() ? s->genomes[g].c_str() : nullptr; }
size_t covh_genome_set_n_contigs(const covh_genome_set *s) { return s ? s->genome_of.size() : 0; }

void covh_genome_set_contig(const covh_genome_set *s, size_t i, const char **name, int32_t *genome) {
    const bool ok = s && i < s->genome_of.size();
    if (name) *name = ok ? s->name(i) : nullptr;
    if (genome) *genome = ok ? s->genome_of[i] : -1;
}

int32_t covh_genome_set_genome_of(const covh_genome_set *s, const char *contig, size_t len) {
    if (!s || !contig || s->genome_of.empty()) return -1;
    for (uint64_t h = hash_name(contig, len) & s->mask;; h = (h + 1) & s->mask) {
        const uint32_t slot = s->table[h];
        if (!slot) return -1;
        const size_t c = slot - 1;
        if (s->len(c) == len && !memcmp(s->name(c), contig, len)) return s->genome_of[c];
    }
}

size_t covh_genome_set_genome_of_tid(const covh_genome_set *s, const covh_header *h, int32_t *out) {
    size_t found = 0;
    for (uint32_t t = 0; t < h->n_targets; t++) {
        out[t] = covh_genome_set_genome_of(s, h->names + h->name_off[t], h->name_off[t + 1] - h->name_off[t]);
        found += out[t] >= 0;
    }
    return found;
}

void covh_genome_set_free(covh_genome_set *s) { delete s; }

}  // extern "C"
