"""A plain-Python BAM reader for the truth BAM's tests (tests/test_truth_bam_host.py, tests/test_gpu_truth_bam.py): it walks the
BGZF members itself and checks each one against zlib, parses the header and the records with struct, and renders every record
as the 13 columns of the truth SAM's line (the 11 fields, NM:i: and MD:Z:), next to the raw fields the tests check directly.
Not a test; nothing here needs a GPU or any tool outside the standard library."""
import struct
import zlib

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def bgzf_members(blob):
    """[(member bytes, inflated bytes)] of a BGZF file; asserts the framing: gzip magic, FLG.FEXTRA, the BC subfield with BSIZE,
    a member of at most 65536 bytes that inflates to at most 65536, CRC-32 and ISIZE as zlib computes them, and the
    specification's 28-byte end-of-file block at the end."""
    assert len(blob) >= 28 and blob[-28:] == BGZF_EOF, "no BGZF end-of-file block"
    out, o = [], 0
    while o < len(blob):
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", blob, o)
        assert (id1, id2, cm) == (31, 139, 8) and flg & 4, "not a BGZF member at byte %d" % o
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si1, si2, slen = struct.unpack_from("<BBH", blob, x)
            if (si1, si2) == (66, 67):
                assert slen == 2
                bsize = struct.unpack_from("<H", blob, x + 4)[0] + 1
            x += 4 + slen
        assert x == o + 12 + xlen and bsize is not None, "no BC subfield at byte %d" % o
        assert bsize <= 65536 and o + bsize <= len(blob)
        data = zlib.decompress(blob[o + 12 + xlen:o + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", blob, o + bsize - 8)
        assert len(data) <= 65536 and isize == len(data) and crc == zlib.crc32(data), "member at byte %d: CRC-32 / ISIZE" % o
        out.append((blob[o:o + bsize], data))
        o += bsize
    assert o == len(blob) and out[-1][1] == b""
    return out


def reg2bin(beg, end):
    """SAM specification, section 5.3: the bin of the 0-based half-open region [beg, end)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def parse_record(buf, o=0, names=None):
    """The record at buf[o:] -> (dict, offset behind it).  dict: "cols" = the SAM line's 13 columns (RNAME from `names`, or the
    number as text without them), the raw fields, "seq_bytes" (the packed SEQ) and "tags" = [(tag, type, value)]."""
    block_size, ref, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", buf, o)
    end = o + 4 + block_size
    x = o + 36
    name = buf[x:x + l_name]
    assert name[-1:] == b"\0" and b"\0" not in name[:-1]
    x += l_name
    ops = struct.unpack_from("<%dI" % n_cig, buf, x)
    x += 4 * n_cig
    cigar = "".join("%d%s" % (v >> 4, CIGAR_OPS[v & 15]) for v in ops)
    seq_bytes = buf[x:x + (l_seq + 1) // 2]
    x += (l_seq + 1) // 2
    seq = "".join(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15] for b in seq_bytes)[:l_seq]
    qual = "".join(chr(q + 33) for q in buf[x:x + l_seq])
    raw_qual = bytes(buf[x:x + l_seq])
    x += l_seq
    tags = []
    while x < end:
        tag, typ = buf[x:x + 2].decode(), chr(buf[x + 2])
        x += 3
        if typ == "Z":
            z = buf.index(b"\0", x)
            tags.append((tag, typ, buf[x:z].decode()))
            x = z + 1
        else:
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[typ]
            tags.append((tag, typ, struct.unpack_from(fmt, buf, x)[0]))
            x += struct.calcsize(fmt)
    assert x == end, "the tags do not end with the record"
    rname = lambda r: "*" if r < 0 else (names[r] if names is not None else str(r))
    rnext = "*" if nref < 0 else ("=" if nref == ref else rname(nref))
    cols = [name[:-1].decode(), str(flag), rname(ref), str(pos + 1), str(mapq), cigar, rnext, str(npos + 1), str(tlen), seq, qual]
    cols += ["%s:%s:%s" % (t, "i" if ty in "cCsSiI" else ty, v) for t, ty, v in tags]
    span = sum(v >> 4 for v in ops if (v & 15) in (0, 2, 3, 7, 8))
    rec = dict(cols=cols, block_size=block_size, length=end - o, refID=ref, pos=pos, l_read_name=l_name, mapq=mapq, bin=bin_, n_cigar_op=n_cig,
               flag=flag, l_seq=l_seq, next_refID=nref, next_pos=npos, tlen=tlen, seq_bytes=bytes(seq_bytes), raw_qual=raw_qual, tags=tags, span=span)
    return rec, end


def read_bam(path):
    """-> dict(text = the header text, refs = [(name, length)], records = [parse_record's dicts], members = number of BGZF
    members, the end-of-file block included).  Every assertion of bgzf_members holds for the file."""
    blob = open(path, "rb").read()
    members = bgzf_members(blob)
    buf = b"".join(d for _, d in members)
    assert buf[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", buf, 4)[0]
    text = buf[8:8 + l_text].decode()
    o = 8 + l_text
    n_ref = struct.unpack_from("<i", buf, o)[0]
    o += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", buf, o)[0]
        nm = buf[o + 4:o + 4 + l_name]
        assert nm[-1:] == b"\0"
        refs.append((nm[:-1].decode(), struct.unpack_from("<i", buf, o + 4 + l_name)[0]))
        o += 8 + l_name
    names = [r[0] for r in refs]
    records = []
    while o < len(buf):
        rec, o = parse_record(buf, o, names)
        records.append(rec)
    assert o == len(buf)
    return dict(text=text, refs=refs, records=records, members=len(members), size=len(blob))
