"""Builders the tag-window tests share (test_gpu_{bam,sam,sam_bam,bam_sam}_window.py, test_gpu_tag_directions.py): inputs and the
plain decoding of outputs.  What a test expects -- its `expected`, `check` and restatements -- stays in its own file."""
import gzip
import random
import struct
import zlib

NIB = b"=ACMGRSVTWYHKDBN"
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _bgzf(data, block=0xff00, level=6):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def inflate(members):
    return gzip.decompress(members + EOF) if members else b""


def patterns31(mk, n=200, seed=3):
    rnd = random.Random(seed)
    return mk.parse_pattern_list(kmer_seq=[bytes(rnd.choice(b"ACGT") for _ in range(31)) for _ in range(n)])


def bam_record(name, seq, qual=None, aux=b"", cigar=(), ref=0, pos=100, flag=0, mapq=60, nref=-1, npos=-1, tlen=0):
    """block_size + one BAM record; seq in the 16-letter alphabet, qual = l_seq raw bytes (default: 30s)"""
    l = len(seq)
    packed = bytearray((l + 1) // 2)
    for k, ch in enumerate(seq):
        packed[k >> 1] |= NIB.index(ch) << (4 if k % 2 == 0 else 0)
    qual = bytes([30] * l) if qual is None else qual
    assert len(qual) == l
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, mapq, 4680, len(cigar), flag, l, nref, npos, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + qual + aux
    return struct.pack("<i", len(body)) + body


def records_of(text, last=True):
    """the line rule: -> [(line without its line end, name, SEQ as the matcher sees it, existing-field scan input)], bytes used"""
    used = len(text) if last or text.endswith(b"\n") else text.rfind(b"\n") + 1
    out = []
    for ln in text[:used].split(b"\n"):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln or ln[:1] == b"@":
            continue
        f = ln.split(b"\t")
        assert len(f) >= 10
        seq = b"" if f[9] == b"*" else bytes(c - 32 if 97 <= c <= 122 else c for c in f[9])
        out.append((ln, f[0], seq, f[11:]))
    return out, used


def existing_value(aux, tag):
    """SamFile::find_tag: the first optional field of at least 5 bytes that starts with tag ':' -> its value (None: no such field)"""
    for f in aux:
        if len(f) >= 5 and f[:2] == tag and f[2:3] == b":":
            assert f[3:5] == b"Z:"
            return f[5:]
    return None
