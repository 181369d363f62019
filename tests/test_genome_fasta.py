"""Genomes defined by FASTA files (`coverm genome -f / -d -x / --genome-fasta-list`; genome_parsing.rs:10-70,
genomes_and_contigs.rs:25-40) through the C ABI (covh_genome_fasta_paths, covh_genome_set_*) and the binary's argument
handling.  Fixtures: the reference's FASTA fixtures under tests/golden/fasta; synthetic FASTA is written into tmp_path."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

from coverm_amd import host
from tests.fixtures import FIXDIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA = os.path.join(ROOT, "tests", "golden", "fasta")
BIN = os.path.join(ROOT, "coverm_amd", "coverm-amd")


def definition_pairs(name):
    rows = []
    for line in open(os.path.join(FIXDIR, name)):
        g, c = line.rstrip("\n").split("\t")
        rows.append((g, c))
    return rows


def resolve(paths, full=False, threads=1):
    gs = host.GenomeSet(paths, use_full_contig_names=full, threads=threads)
    return gs.genomes, gs.pairs()


def error_of(paths, full=False, threads=1):
    with pytest.raises(host.GenomeFastaError) as ei:
        host.GenomeSet(paths, use_full_contig_names=full, threads=threads)
    return str(ei.value)


def write(path, data):
    with open(path, "wb") as fh:
        fh.write(data if isinstance(data, bytes) else data.encode())
    return str(path)


# ---------------------------------------------------------------------------------------------------------------- fixtures
def test_genomes_dir_7seqs_equals_7seqs_definition():
    paths = host.genome_fasta_directory(os.path.join(FASTA, "genomes_dir_7seqs"), "fasta")
    assert [os.path.basename(p) for p in paths] == ["genome%d.fasta" % i for i in range(1, 7)]
    genomes, pairs = resolve(paths)
    assert genomes == ["genome%d" % i for i in range(1, 7)]
    assert pairs == definition_pairs("7seqs.definition")


@pytest.mark.parametrize("ext", ["fna", ".fna"])
def test_genomes_dir_extension_filters_files(ext):
    paths = host.genome_fasta_directory(os.path.join(FASTA, "genomes_dir"), ext)
    assert [os.path.basename(p) for p in paths] == ["seq1.fna", "seq2.fna"]      # not_a_genome, not_a_genome.extension skipped
    assert resolve(paths) == (["seq1", "seq2"], [("seq1", "seq1"), ("seq2", "seq2")])


def test_genomes_dir_compressed():
    paths = host.genome_fasta_directory(os.path.join(FASTA, "genomes_dir_compressed"), "fna.gz")
    assert [os.path.basename(p) for p in paths] == ["seq1.fna.gz", "seq2.fna.gz"]
    assert resolve(paths) == resolve(host.genome_fasta_directory(os.path.join(FASTA, "genomes_dir")))


def test_2seqs_split_genomes_equals_its_definition():
    paths = host.genome_fasta_directory(os.path.join(FASTA, "2seqs_split_genomes"))
    assert resolve(paths)[1] == definition_pairs("2seqs.genome-definition")


def test_directory_order_is_bytewise_and_symlinks_are_followed(tmp_path):
    d = tmp_path / "d"
    d.mkdir()
    for n in ("b.fna", "B.fna", "a.fna", "_x.fna"):
        write(d / n, ">%s_c\nACGT\n" % n[:-4])
    os.symlink(str(d / "a.fna"), str(d / "link.fna"))       # same contig as a.fna: resolving it shows it was listed
    os.symlink(str(tmp_path / "missing"), str(d / "dangling.fna"))
    (d / "sub.fna").mkdir()
    paths = host.genome_fasta_directory(str(d), "fna")
    assert [os.path.basename(p) for p in paths] == ["B.fna", "_x.fna", "a.fna", "b.fna", "link.fna"]
    assert "at least 'a' and 'link'" in error_of(paths)


def test_empty_directory_and_missing_directory_are_errors(tmp_path):
    (tmp_path / "e").mkdir()
    write(tmp_path / "e" / "x.fa", ">c\nA\n")
    with pytest.raises(IOError, match="No genome FASTA files with extension .fna"):
        host.genome_fasta_directory(str(tmp_path / "e"))
    with pytest.raises(IOError, match="Unable to read genome FASTA directory"):
        host.genome_fasta_directory(str(tmp_path / "nope"))


# ---------------------------------------------------------------------------------------------------------------- names
@pytest.mark.parametrize("name,stem", [("a.b.fna", "a.b"), ("x.fna.gz", "x"), ("x.fna.bz2", "x"), (".hidden", ".hidden"),
                                       ("plain", "plain"), ("y.fa.xz", "y")])
def test_genome_name_is_the_file_stem(tmp_path, name, stem):
    # (the format comes from the bytes: the .bz2 / .xz files here hold plain text)
    p = write(tmp_path / name, gzip.compress(b">c\nA\n") if name.endswith(".gz") else b">c\nA\n")
    assert resolve([p])[0] == [stem]


def test_gz_inside_a_directory_name_cuts_the_path_there(tmp_path):
    """genome_parsing.rs:23-31 cuts the whole path string at its last ".gz": a directory name holding one decides the name."""
    d = tmp_path / "bins.gzdir"
    d.mkdir()
    p = write(d / "g1.fna", ">c\nA\n")
    assert resolve([p])[0] == ["bins"]


def test_same_stem_from_two_directories_is_an_error(tmp_path):
    for sub in ("a", "b"):
        (tmp_path / sub).mkdir()
        write(tmp_path / sub / "g.fna", ">%s_contig\nACGT\n" % sub)
    e = error_of([str(tmp_path / "a" / "g.fna"), str(tmp_path / "b" / "g.fna")])
    assert e == "The genome name g was derived from >1 file"


# ---------------------------------------------------------------------------------------------------------------- headers
def test_contig_name_is_cut_at_the_first_space_only(tmp_path):
    p = write(tmp_path / "g.fna", ">c1 desc here\nACGT\n>c2\tkept tab\nAC\nGT\n>c3\n>c4  two\nA")
    assert resolve([p])[1] == [("g", "c1"), ("g", "c2\tkept"), ("g", "c3"), ("g", "c4")]
    assert resolve([p], full=True)[1] == [("g", "c1 desc here"), ("g", "c2\tkept tab"), ("g", "c3"), ("g", "c4  two")]


def test_crlf_is_stripped(tmp_path):
    p = write(tmp_path / "g.fna", ">c1 x\r\nACGT\r\n>c2\r\nAC\r\n")
    assert resolve([p])[1] == [("g", "c1"), ("g", "c2")]
    assert resolve([p], full=True)[1] == [("g", "c1 x"), ("g", "c2")]


def test_gt_inside_a_line_is_not_a_record(tmp_path):
    p = write(tmp_path / "g.fna", ">c1 a>b\nAC>GT\n>c2\nA\n")
    assert resolve([p])[1] == [("g", "c1"), ("g", "c2")]


def test_repeated_contig_inside_one_file_is_an_error(tmp_path):
    p = write(tmp_path / "g.fna", ">c1\nA\n>c2\nA\n>c1 again\nA\n")
    assert error_of([p]) == "The contig 'c1' has been assigned to multiple genomes, at least 'g' and 'g'"


def test_contig_name_clashing_fixture():
    paths = [os.path.join(FASTA, "contig_name_clashing", "genome%d.fna" % i) for i in (1, 2, 3)]
    e = error_of(paths)
    assert e == "The contig 'random_sequence_length_500_1' has been assigned to multiple genomes, at least 'genome1' and 'genome2'"


# ---------------------------------------------------------------------------------------------------------------- formats
def _bgzf(data, block=7):
    out = b""
    for i in range(0, len(data), block):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(data[i:i + block]) + c.flush()
        out += (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
                + struct.pack("<II", zlib.crc32(data[i:i + block]) & 0xffffffff, len(data[i:i + block])))
    return out + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_formats_give_identical_results(tmp_path):
    text = b"".join(b">g_c%d some description\n%s\n" % (i, b"ACGT" * (i + 1)) for i in range(200))
    forms = {
        "plain.fna": text,
        "gz.fna.gz": gzip.compress(text),
        "multi.fna.gz": gzip.compress(text[:1001]) + gzip.compress(text[1001:5003]) + gzip.compress(text[5003:]),
        "bgzf.fna.gz": _bgzf(text),
        "noname.fna": gzip.compress(text),           # gzip detected by magic bytes, not by name
    }
    results = []
    for name, data in forms.items():
        d = tmp_path / name.split(".")[0]
        d.mkdir()
        results.append(resolve([write(d / name, data)])[1])
        assert [g for g, _ in results[-1]] == [name.split(".")[0]] * 200
    contigs = [[c for _, c in r] for r in results]
    assert all(c == ["g_c%d" % i for i in range(200)] for c in contigs)


def test_fastq_empty_missing_and_other_compressions_are_errors(tmp_path):
    fq = write(tmp_path / "r.fq", "@r1\nACGT\n+\nIIII\n")
    assert "is not a fasta file, but a Fastq" in error_of([fq])
    empty = write(tmp_path / "e.fna", b"")
    assert error_of([empty]) == "Unable to read fasta file %s: the file is empty" % empty
    assert error_of([write(tmp_path / "ez.fna.gz", gzip.compress(b""))]).endswith(": the file is empty")
    assert error_of([str(tmp_path / "missing.fna")]).startswith("Unable to read fasta file %s" % (tmp_path / "missing.fna"))
    assert "not a fasta file" in error_of([write(tmp_path / "t.fna", "ACGT\n>c\n")])
    for name, magic, fmt in (("b.fna.bz2", b"BZh91AY&SY", "bzip2"), ("x.fna.xz", b"\xfd7zXZ\x00\x00", "xz"),
                             ("z.fna.zst", b"\x28\xb5\x2f\xfd\x00\x00", "zstd")):
        assert "%s-compressed input is not supported" % fmt in error_of([write(tmp_path / name, magic)])
    assert "gzip stream is truncated" in error_of([write(tmp_path / "trunc.fna.gz", gzip.compress(b">c1\nACGT\n" * 50)[:-12])])


def test_first_error_in_file_order(tmp_path):
    """A one-file-at-a-time read: a file's open error comes before the genome name check, its parse error after its contigs."""
    a = write(tmp_path / "a.fna", ">c1\nA\n")
    fq = write(tmp_path / "b.fna", "@r\nA\n+\nI\n")
    dup = write(tmp_path / "c.fna", ">c1\nA\n")
    assert "not a fasta file" in error_of([a, fq, dup])
    assert "at least 'a' and 'c'" in error_of([a, dup, fq])


# ---------------------------------------------------------------------------------------------------------------- list
def test_genome_fasta_list_blank_lines_and_crlf(tmp_path):
    d7 = os.path.join(FASTA, "genomes_dir_7seqs")
    lst = write(tmp_path / "list.txt", "\r\n".join([os.path.join(d7, "genome%d.fasta" % i) for i in (1, 2, 3)]) + "\r\n\r\n\n" +
                "\n".join([os.path.join(d7, "genome%d.fasta" % i) for i in (4, 5, 6)]))
    paths = host.genome_fasta_list(lst)
    assert paths == [os.path.join(d7, "genome%d.fasta" % i) for i in range(1, 7)]
    assert resolve(paths)[1] == definition_pairs("7seqs.definition")
    with pytest.raises(IOError, match="No genome FASTA files were listed"):
        host.genome_fasta_list(write(tmp_path / "blank.txt", "\n\r\n"))


def test_relative_list_paths_are_relative_to_the_working_directory(tmp_path, monkeypatch):
    (tmp_path / "g").mkdir()
    write(tmp_path / "g" / "one.fna", ">c\nA\n")
    lst = write(tmp_path / "list.txt", "g/one.fna\n")
    monkeypatch.chdir(tmp_path)
    assert resolve(host.genome_fasta_list(lst)) == (["one"], [("one", "c")])


# ---------------------------------------------------------------------------------------------------------------- threads
def test_two_thousand_files_identical_for_any_thread_count(tmp_path):
    d = tmp_path / "many"
    d.mkdir()
    for i in range(2000):
        write(d / ("g%04d.fna" % i), "".join(">g%d_c%d len=%d\n%s\n" % (i, k, k, "ACGT" * (k + 1)) for k in range(i % 5 + 1)))
    paths = host.genome_fasta_directory(str(d))
    r1 = resolve(paths, threads=1)
    assert r1 == resolve(paths, threads=8) and len(r1[0]) == 2000 and len(r1[1]) == sum(i % 5 + 1 for i in range(2000))
    gs = host.GenomeSet(paths, threads=8)
    assert list(gs.genome_of_tid(["g7_c1", "nope", "g1999_c0"])) == [7, -1, 1999]
    # two bad files: the first in file order is reported, whichever thread meets its file first
    write(d / "g0500.fna", "@fastq\nA\n+\nI\n")
    write(d / "g1500.fna", ">g3_c0\nA\n")
    for t in (1, 8):
        assert error_of(paths, threads=t) == 'File "%s" is not a fasta file, but a Fastq' % paths[500]
    write(d / "g0500.fna", ">g0500_c0\nA\n")
    for t in (1, 8):
        assert error_of(paths, threads=t) == "The contig 'g3_c0' has been assigned to multiple genomes, at least 'g0003' and 'g1500'"


def test_large_plain_file_scanned_in_ranges(tmp_path):
    """A plain file above two 32 MiB ranges is cut into ranges: headers on and across every boundary are found once."""
    rng_line = b"ACGT" * 30 + b"\n"
    parts, names = [], []
    size, i = 0, 0
    while size < (100 << 20):
        name = b"contig_%d desc" % i
        rec = b">" + name + b"\n" + rng_line * (1 + (i * 7919) % 3000)
        parts.append(rec)
        names.append("contig_%d" % i)
        size += len(rec)
        i += 1
    p = write(tmp_path / "big.fna", b"".join(parts))
    for t in (1, 4):
        genomes, pairs = resolve([p], threads=t)
        assert genomes == ["big"] and [c for _, c in pairs] == names


# ---------------------------------------------------------------------------------------------------------------- binary
def test_binary_rejects_conflicting_genome_sources(tmp_path):
    d = os.path.join(FASTA, "genomes_dir")
    f = os.path.join(d, "seq1.fna")
    lst = write(tmp_path / "l.txt", f + "\n")
    defn = os.path.join(FIXDIR, "2seqs.genome-definition")
    for extra, pair in ((["-f", f, "-d", d], ("--genome-fasta-files", "--genome-fasta-directory")),
                        (["-f", f, "--genome-fasta-list", lst], ("--genome-fasta-files", "--genome-fasta-list")),
                        (["-d", d, "--genome-fasta-list", lst], ("--genome-fasta-directory", "--genome-fasta-list")),
                        (["-d", d, "-s", "~"], ("--genome-fasta-directory", "--separator")),
                        (["--genome-fasta-list", lst, "--single-genome"], ("--genome-fasta-list", "--single-genome")),
                        (["-f", f, "--genome-definition", defn], ("--genome-fasta-files", "--genome-definition")),
                        (["--genome-definition", defn, "-d", d], ("--genome-fasta-directory", "--genome-definition"))):
        p = subprocess.run([BIN, "genome", "-b", "x.bam"] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "the argument '%s' cannot be used with '%s'" % pair in p.stderr, (extra, p.stderr)
        assert p.stdout == ""


def test_binary_genome_flags_are_unknown_in_contig_mode():
    for flag in ("-f", "--genome-fasta-files", "-d", "--genome-fasta-directory", "-x", "--genome-fasta-list", "--use-full-contig-names"):
        p = subprocess.run([BIN, "contig", "-b", "x.bam", flag, "y"], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "unknown argument " + flag in p.stderr, (flag, p.stderr)


def test_binary_without_any_genome_source_keeps_its_message():
    p = subprocess.run([BIN, "genome", "-b", "x.bam", "-x", "fna"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "genome mode over BAM files needs --separator, --single-genome or --genome-definition\n" in p.stderr
