"""The FASTA files the input side is checked on, with a reference parser and the chunk borders each file puts where, shared by the
CPU tests (tests/test_fasta_host.py: the host parser and its .fai against the reference; the table reaches every kind of border)
and the GPU tests (tests/test_gpu_staging.py: the device parser, the slice gather and the genome index against the reference).

The reference is written from the rule, not from either C++ parser: a file is lines split on "\\n"; one trailing "\\r" of a line is
dropped; an empty line and a line that starts with ";" are nothing; a line that starts with ">" opens a record; every byte of every
other line is a base; bases before the first header are an error.  A "\\r" anywhere else is therefore a base (one that is not ACGT).

Every case is at most 2 KB (one_long_line: 5 KB) and names what it is for.  At the end: the genomes of the index, has_n and slice
tests and their numpy references."""
import functools
import re

import numpy as np

SEQUENCE_BEFORE_HEADER = "sequence before header"


class Refused(ValueError):
    pass


# ---------------------------------------------------------------- the reference
def index_name(header):
    """the record's name as the library reports it: the header's first word, from behind its first "chrom" (else its first "chr") on"""
    word = re.split(rb"[ \t]", header, maxsplit=1)[0]
    for key in (b"chrom", b"chr"):
        i = word.find(key)
        if i >= 0:
            return word[i + len(key):]
    return word


def parse(data):
    """[(header text, bases)] of a file's bytes"""
    recs = []
    for line in data.split(b"\n"):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b";"):
            continue
        if line.startswith(b">"):
            recs.append((line[1:], bytearray()))
        elif not recs:
            raise Refused(SEQUENCE_BEFORE_HEADER)
        else:
            recs[-1][1].extend(line)
    return [(h, bytes(s)) for h, s in recs]


_CODE = np.full(256, 4, np.uint8)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _CODE[list(_pair)] = _i


def codes_of(seq):
    """A a -> 0, C c -> 1, G g -> 2, T t -> 3, anything else 4"""
    return _CODE[np.frombuffer(bytes(seq), np.uint8)]


def fnv1a_upper(seq):
    """scs_fasta_probe's checksum: FNV-1a's multiply-and-xor over the bases with a..z upper-cased, from the library's own start value"""
    h = 1469598103934665603
    for b in seq:
        h = ((h ^ (b - 32 if 97 <= b <= 122 else b)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class Parsed:
    def __init__(self, data):
        recs = parse(data)
        self.headers = [h for h, _ in recs]
        self.names = [index_name(h).decode("latin-1") for h, _ in recs]
        self.lens = [len(s) for _, s in recs]
        self.seq = b"".join(s for _, s in recs)
        self.total = len(self.seq)
        self.codes = codes_of(self.seq)
        self.checksum = fnv1a_upper(self.seq)


def fai(data):
    """The index both writers leave beside the file (fastahack's format), stated from the file's bytes: per record the header's text
    up to its first blank, the record's length, the offset of the first line behind the header that is no comment line, and that
    line's bases and bytes (0 and 0, at the offset where the record ends, when the record has no such line)."""
    lines, off = [], 0                                   # (offset, bytes with the line end, text without it)
    for raw in data.split(b"\n"):
        n = len(raw) + (1 if off + len(raw) < len(data) else 0)
        if n:
            lines.append((off, n, raw[:-1] if raw.endswith(b"\r") else raw))
        off += len(raw) + 1
    out, lens = [], iter(Parsed(data).lens)
    for i, (_, _, text) in enumerate(lines):
        if not text.startswith(b">"):
            continue
        k = i + 1
        while k < len(lines) and lines[k][2].startswith(b";"):
            k += 1
        if k < len(lines) and not lines[k][2].startswith(b">"):
            first = (lines[k][0], len(lines[k][2]), lines[k][1])
        else:
            first = (lines[k][0] if k < len(lines) else len(data), 0, 0)
        out.append(b"%s\t%d\t%d\t%d\t%d\n" % ((text[1:].split(b" ")[0], next(lens)) + first))
    return b"".join(out)


# ---------------------------------------------------------------- the table
def _bases(n, seed, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, np.uint8)[np.random.default_rng(seed).integers(0, len(alphabet), n)])


def _wrap(seq, width, eol=b"\n", last_eol=None):
    lines = [seq[i:i + width] for i in range(0, len(seq), width)]
    return eol.join(lines) + (eol if last_eol is None else last_eol) if lines else b""


def _two_records(eol, last_eol=None):
    return b">chr20_1_333" + eol + _wrap(_bases(333, 1), 60, eol) + b">chr20_2_250" + eol + _wrap(_bases(250, 2), 60, eol, last_eol)


def _ragged():
    seq, out, o = _bases(1500, 7, b"ACGTN"), [b">chrom4_1_1500\n"], 0
    for i in range(10 ** 6):
        if o >= len(seq):
            break
        w = (1, 13, 100, 57)[i % 4]
        out.append(seq[o:o + w] + b"\n"); o += w
    return b"".join(out)


def _all_bytes():
    vals = bytes(v for v in range(1, 256) if v != 10)        # '\r', '>' and ';' among them, each in the middle of a line
    body = b"".join(b"G" + vals[i:i + 40] + b"T\n" for i in range(0, len(vals), 40))
    return b">every_byte\n" + body + b">tail\nAC\n"


# name -> (builder, what it is for); refused cases are listed in REFUSED
CASES = {
    "lf": (lambda: _two_records(b"\n"), "LF line ends, two records of 60-column lines"),
    "crlf": (lambda: _two_records(b"\r\n"), "CRLF line ends: a border between '\\r' and '\\n', and behind '\\r\\n'"),
    "crlf_no_final_newline": (lambda: _two_records(b"\r\n", b""), "CRLF, the last line without a line end: the file ends inside a sequence line"),
    "header_description": (lambda: b">chr7_1_130 the first haplotype, with words\n" + _wrap(_bases(130, 3), 50) + b">x second\nACGTT\n",
                           "a header with a description: the name ends at the first blank"),
    "acgt_in_header_and_comment": (lambda: b";ACGT ACGT a file comment, TTTT\n>ACGT_GATTACA ACGTACGT CCCC\n;GGGG ACGT in a comment\n" + _wrap(_bases(90, 4), 30) +
                                   b">TAG_CAT GATTACA\nACGT\n;ACGTACGTACGT\nTTGA\n", "header and comment lines whose text holds ACGT: a chunk that starts inside one must not keep it"),
    "comments": (lambda: b">a_1_40\n;a comment inside a record\n" + _wrap(_bases(20, 5), 10) + b";another one\n;and a third\n" + _wrap(_bases(20, 6), 10) +
                 b";a comment before a header\n>b_1_12\nACGTACGTACGT\n", "a comment line inside a record, several in a row, and one before a header"),
    "blank_lines": (lambda: b"\n\r\n>c_1_24\nACGTAC\n\nGTACGT\n\r\nACGTACGTACGT\n\n\n", "blank lines (LF and CRLF) at the start, inside a record and at the end"),
    "blank_line_behind_header": (lambda: b">d_1_8\n\nACGTACGT\n>e_1_4\n;c\n\nACGT\n", "a blank line as the first line behind a header: the index line's 0 bases in 1 byte"),
    "empty_records": (lambda: b">f_1_6\nACGTAC\n>empty_middle\n>g_1_3\nACG\n>empty_end\n", "an empty record in the middle and one at the end"),
    "empty_record_no_newline": (lambda: b">h_1_5\nACGTA\n>empty_end", "an empty record whose header ends the file without a line end"),
    "one_long_line": (lambda: b">long_1_5000\n" + _bases(5000, 8) + b"\n>short\nAC\n", "a record on one 5000-base line (5 KB: the one case above 2 KB)"),
    "ragged": (_ragged, "line widths 1, 13, 100, 57, 1, ... with N among the bases"),
    "lower_case": (lambda: b">chr1_1_200\n" + _wrap(_bases(200, 9, b"ACGTacgtNn"), 70), "lower case and N: codes fold the case, the checksum upper-cases"),
    "all_bytes": (_all_bytes, "every byte value 1..255 but '\\n' inside sequence lines, '>' ';' and '\\r' in the middle of a line"),
    "one_base_line": (lambda: b">i_1_1\nA\n>j_1_9\nACGT\nC\nGTAC\n", "a line that is one base, as a whole record and among other lines"),
    "one_header": (lambda: b">lonely_1_0\n", "a file that is one header: one record of no bases"),
    "cr_inside_line": (lambda: b">k_1_5\nAC\rGT\nACGT\n", "AC\\rGT\\n: a '\\r' in the middle of a line is a base that is not ACGT"),
    "cr_twice_at_line_end": (lambda: b">l2_1_5\nACGT\r\r\nTTGA\r\n", "ACGT\\r\\r\\n: only the '\\r' in front of the '\\n' belongs to the line end"),
    "cr_at_file_end": (lambda: b">m_1_8\nTTGA\nACGT\r", "ACGT\\r as the file's last bytes: the '\\r' in front of the end of the file is dropped"),
    "sequence_before_header": (lambda: b";a comment is fine\n\nACGT\n>late_1_2\nAC\n", "bases before the first header: refused"),
}
REFUSED = {"sequence_before_header": SEQUENCE_BEFORE_HEADER}
CR_CASES = ("cr_inside_line", "cr_twice_at_line_end", "cr_at_file_end")
SIZE_CAP = {"one_long_line": 5100}

CHUNKS = (None, 1, 2, 3, 5, 7, 64, 256, 257)                 # SCS_TEST_FASTA_CHUNK of the parser tests; None: unset
SMALL_CHUNKS = (2, 3, 5, 7)


@functools.lru_cache(None)
def data(name):
    return CASES[name][0]()


@functools.lru_cache(None)
def parsed(name):
    return Parsed(data(name))


# ---------------------------------------------------------------- where a chunk size puts its borders
BORDER_KINDS = ("behind_newline_then_header",    # right behind a '\n', the next chunk starts with the '>' of a header
                "behind_newline_then_comment",   # ... with the ';' of a comment line
                "inside_header_before_acgt",     # inside a header line, A C G T (either case) in the part of it the next chunk starts with
                "inside_comment_before_acgt",    # the same inside a comment line
                "between_cr_and_lf",             # '\r' ends a chunk, its '\n' starts the next
                "last_byte_without_newline",     # the file has no final newline and its last byte is a chunk of its own
                "behind_the_header_mark")        # the '>' of a header ends a chunk: the mark and the header's text lie in two chunks


def borders(d, chunk):
    """{offset: set of kinds} of the chunk borders of d under chunks of `chunk` bytes (a border at o: one chunk ends with byte o - 1,
    the next starts with byte o), for the borders that are of one of BORDER_KINDS"""
    starts = [0] + [i + 1 for i, b in enumerate(d) if b == 10 and i + 1 < len(d)]
    line_of = np.zeros(len(d), np.int64)
    line_of[starts[1:]] = 1
    line_of = np.cumsum(line_of)
    out = {}
    for o in range(chunk, len(d), chunk):
        s = starts[line_of[o]]
        end = d.find(b"\n", o)
        rest = d[o:end if end >= 0 else len(d)]
        kinds = set()
        if s == o and d[o] == ord(">"):
            kinds.add("behind_newline_then_header")
        if s == o and d[o] == ord(";"):
            kinds.add("behind_newline_then_comment")
        if s < o and d[s] in b">;" and any(b in rest for b in b"ACGTacgt"):
            kinds.add("inside_header_before_acgt" if d[s] == ord(">") else "inside_comment_before_acgt")
        if d[o - 1] == 13 and d[o] == 10:
            kinds.add("between_cr_and_lf")
        if o == len(d) - 1 and d[-1] != 10:
            kinds.add("last_byte_without_newline")
        if s == o - 1 and d[s] == ord(">"):
            kinds.add("behind_the_header_mark")
        if kinds:
            out[o] = kinds
    return out


def kinds_reached(chunk, names=None):
    """{kind: [case, ...]} over the table (the refused cases left out) at one chunk size"""
    reach = {k: [] for k in BORDER_KINDS}
    for name in (names or CASES):
        if name not in REFUSED:
            for k in set().union(*borders(data(name), chunk).values()):
                reach[k].append(name)
    return reach


# ---------------------------------------------------------------- the ragged 100 KB file of the whole-job test, for chunks of 4096 and 65536
def ragged_100k():
    """the text of test_fasta_parsed_on_the_device_handles_ragged_text (tests/test_gpu_parity.py), byte for byte"""
    rng = np.random.default_rng(12)
    rnd = lambda n: "".join(rng.choice(list("ACGTacgtN"), size=n, p=[0.24, 0.2, 0.2, 0.24, 0.03, 0.03, 0.02, 0.02, 0.02]))
    a, b, c = rnd(30011), rnd(40000), rnd(25000)
    f = [b"\r\n>chr3_1_30011 first haplotype\r\n"]
    for i in range(0, len(a), 70):
        f.append(a[i:i + 70].encode() + b"\r\n")
        if i == 700:
            f.append(b";a comment line in the middle of a record\r\n\r\n")
    f.append(b">3_2_40000\n" + b.encode() + b"\n")
    f.append(b";comment before a header\n>chrom4_1_25000\n")
    w = 0
    for step in [13, 100, 1, 57] * 1000:
        if w >= len(c):
            break
        f.append(c[w:w + step].encode() + b"\n"); w += step
    f.append(b">4_2_9")
    return b"".join(f)


RAGGED_CHUNKS = (4096, 65536)


# ---------------------------------------------------------------- the genome index against numpy
INDEX_TOTALS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)


INDEX_VARIANTS = ("n_60_to_70", "n_63_alone", "n_64_alone")


def index_genome(total, variant):
    """`total` bases: random ACGT in both cases with a few other bytes; N at 0 and over the last base; and, as far as the genome
    reaches, a run of N over 60..70 (across a word border), or an N at 63 alone, or at 64 alone (its neighbours ACGT)"""
    rng = np.random.default_rng([total, INDEX_VARIANTS.index(variant)])
    g = np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, total)].copy()
    other = rng.random(total) < 0.03
    g[other] = np.frombuffer(b"NnRY-*\r.", np.uint8)[rng.integers(0, 8, int(other.sum()))]
    g[0] = ord("N")
    if variant == "n_60_to_70":
        g[60:70] = ord("N")
    else:
        g[58:70] = np.frombuffer(b"ACGTacgtACGT", np.uint8)[:len(g[58:70])]
        at = 63 if variant == "n_63_alone" else 64
        g[at:at + 1] = ord("N")
    g[total - 1] = ord("N")
    return g.tobytes()


def split_three(total):
    """three record lengths that add up to total, the two inner borders not on a multiple of 16 (where the total allows it)"""
    if total < 3:
        return [total]
    a = max(1, total // 3) | 1
    b = max(a + 1, (2 * total) // 3)
    if b % 16 == 0:
        b += 3
    b = min(b, total - 1)
    return [a, b - a, total - b]


def popcount64(a):
    return np.unpackbits(np.ascontiguousarray(a, "<u8").view(np.uint8)).reshape(-1, 64).sum(axis=1).astype(np.uint64) if len(a) else np.zeros(0, np.uint64)


def index_reference(codes):
    """what scs_download_genome must return for these base codes: dict of gc_bits, n_bits, gc_pref, n_pref, gc_pair, g2"""
    n = len(codes)
    nw = (n + 63) // 64
    pad = np.zeros(nw * 64, np.uint8)
    pad[:n] = codes
    bits = lambda mask: np.concatenate([np.packbits(mask, bitorder="little").view("<u8").astype(np.uint64), np.zeros(1, np.uint64)])
    gc_mask = (pad == 1) | (pad == 2)
    gc_mask[n:] = False
    gc, nb = bits(gc_mask), bits(np.concatenate([codes > 3, np.zeros(nw * 64 - n, bool)]))
    pref = lambda b: np.concatenate([np.zeros(1, np.uint64), np.cumsum(popcount64(b[:-1]), dtype=np.uint64)])
    two = (pad & 3).astype(np.uint32)
    two[pad > 3] = 0
    g2 = np.zeros(nw * 4, np.uint32)
    for k in range(16):
        g2 |= two[k::16] << np.uint32(2 * k)
    r = dict(gc_bits=gc, n_bits=nb, gc_pref=pref(gc), n_pref=pref(nb), g2=g2)
    r["gc_pair"] = np.stack([r["gc_bits"], r["gc_pref"]], axis=1)
    return r


INDEX_KEYS = ("gc_bits", "n_bits", "gc_pref", "n_pref", "gc_pair", "g2")


def check_index(got, codes, what):
    """codes and every index array of a download against numpy, exactly; word nwords of the bit arrays is zero"""
    assert got["codes"].dtype == np.uint8 and np.array_equal(got["codes"], codes), "%s: codes differ, the first at %s" % (what, np.flatnonzero(got["codes"][:len(codes)] != codes[:len(got["codes"])])[:1])
    want = index_reference(codes)
    for k in INDEX_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs in %d of %d entries, the first at %d" % (what, k, bad.size, len(want[k]), bad[0])
    assert got["gc_bits"][-1] == 0 and got["n_bits"][-1] == 0, what


# ---------------------------------------------------------------- has_n
HASN_SEED = 11


def hasn_genome():
    """Four records of a few tens of kb; N blocks in the first and the third, none in the second and the last.  Record ends on
    multiples of 64 of the global coordinate (25600, 38400) and off them."""
    out = []
    for k, (n, blocks) in enumerate(((25600, ((0, 10), (5000, 5300), (25590, 25600))), (12800, ()), (70001, ((100, 101), (33333, 34000), (69990, 70001))), (11007, ()))):
        g = np.frombuffer(_bases(n, 40 + k), np.uint8).copy()
        for a, b in blocks:
            g[a:b] = ord("N")
        out.append(("n%d_1_%d" % (k, n), g.tobytes()))
    return out


# ---------------------------------------------------------------- the slice path
SLICE_LENS = (30030, 20020, 13131)
SLICE_CHUNKS = (150, 256, 1000)
SLICE_SHARDS = (2, 3, 5)
SLICE_SEED = 3


def slice_records(lens=SLICE_LENS):
    return [("s%d_1_%d" % (k, n), _bases(n, 60 + k, b"ACGTacgtN")) for k, n in enumerate(lens)]


def long_line_records():
    """each record on one line; the first line (5001 bytes) is longer than a piece buffer of 256 bytes.  Three records, so that with two
    shards neither rank's fragments span the whole genome."""
    return [("long_1_5000", _bases(5000, 70, b"ACGTN")), ("mid_1_3000", _bases(3000, 71)), ("tail_1_2500", _bases(2500, 72, b"ACGTacgt"))]


def fasta_text(records, width=70, eol=b"\n", final_newline=True, widths=None):
    """records as FASTA of `width`-column lines; widths: a cycle of line widths instead"""
    out = []
    for name, seq in records:
        out.append(b">" + name.encode() + eol)
        lines, o, i = [], 0, 0
        while o < len(seq):
            w = widths[i % len(widths)] if widths else width
            lines.append(seq[o:o + w]); o += w; i += 1
        if lines:
            out.append(eol.join(lines) + eol)
    text = b"".join(out)
    return text if final_newline else text[:-len(eol)]


def fai_regular(records, width=70, eol=b"\n"):
    """the index of fasta_text(records, width, eol), stated from the records"""
    out, off = [], 0
    for name, seq in records:
        off += 1 + len(name) + len(eol)
        out.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, min(width, len(seq)), min(width, len(seq)) + len(eol)))
        off += len(seq) + ((len(seq) + width - 1) // width) * len(eol)
    return "".join(out)
