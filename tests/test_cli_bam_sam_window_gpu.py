"""`merkurio tag` with BAM input and SAM / STDOUT output formats a window's kept records as SAM lines on the device
(mk_tag_bam_sam_window, cli/tag_windows.cpp: tag_bam_sam_windows_on_device) unless --host-ingest asks for the host loop: both must
give the same output byte for byte (apart from the command line in the writer's own @PG header line), the same text log body, the
same stable parts of the JSON log, and the same errors.  Under MERKURIO_TIMING=1 the window path prints a row of its own, which is
how these tests know which path ran."""
import os
import random
import struct
import subprocess
import zlib

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
WINDOW_ROW = b"BAM -> SAM text windows on the device"
NIB = b"=ACMGRSVTWYHKDBN"
EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
REFS = [(b"1", 100000000), (b"2", 100000000), (b"MT", 16569)]
HEADER = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


def run(args, check=True):
    env = dict(os.environ)
    env["MERKURIO_TIMING"] = "1"
    p = subprocess.run([BIN] + args, capture_output=True, env=env)
    if check and p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    return p


def bgzf(data, block=0xff00):
    out = bytearray()
    for b in range(0, len(data), block):
        chunk = data[b:b + block]
        co = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(payload) + 8 - 1) + payload
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return bytes(out)


def bam_record(name, seq, qual, aux, cigar, ref, pos, flag, mapq, nref, npos, tlen):
    l = len(seq)
    packed = bytearray((l + 1) // 2)
    for k, ch in enumerate(seq):
        packed[k >> 1] |= NIB.index(ch) << (4 if k % 2 == 0 else 0)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, mapq, 4680, len(cigar), flag, l, nref, npos, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + qual + aux
    return struct.pack("<i", len(body)) + body


def make_records(rnd, kmers, n):
    recs = []
    for i in range(n):
        L = rnd.choice((50, 150, 151))
        s = bytearray(rnd.choice(b"ACGTN") for _ in range(L))
        if i % 4 == 0:
            o = rnd.randrange(L - 31)
            s[o:o + 31] = rnd.choice(kmers)
        qual = b"\xff" * L if i % 17 == 0 else bytes(rnd.randrange(0, 94) for _ in range(L))
        aux = [b"NMi" + struct.pack("<i", rnd.randrange(-3, 70000)), b"def" + struct.pack("<f", rnd.randrange(1000) / 1024.0), b"RGZg%d\0" % (i % 3),
               b"XBBs" + struct.pack("<ihhh", 3, 1, -2, 3), b"XFf" + struct.pack("<f", 131072.5), b"XAAc"][:i % 7]
        if i % 1000 == 0:
            aux.append(b"kmZOLD\0")
        ref = rnd.choice((-1, 0, 1, 2, 5))
        recs.append(bam_record(b"r%d" % i, bytes(s), qual, b"".join(aux), (rnd.randrange(1, 40) << 4 | 4, L << 4, 3 << 4 | 2) if i % 5 else (), ref,
                               rnd.randrange(-1, 10 ** 8), rnd.choice((99, 147, 0, 16, 4)), rnd.randrange(61), rnd.choice((-1, ref, 2)), rnd.randrange(-1, 10 ** 8),
                               rnd.randrange(-500, 500)))
    return recs


def write_bam(path, recs, cut=0):
    """header + records as BGZF members that end anywhere; cut: that many bytes of the last record are missing"""
    text = b"BAM\1" + struct.pack("<i", len(HEADER)) + HEADER + struct.pack("<i", len(REFS))
    for nm, ln in REFS:
        text += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    text += b"".join(recs)
    if cut:
        text = text[:-cut]
    open(path, "wb").write(bgzf(text) + EOF)


def log_body(path):
    return open(path, "rb").read().split(b"\n", 4)[4]


def json_stable(path):
    t = open(path, "rb").read()
    head, rest = t.split(b'  "meta_information": ', 1)
    key = b'  "pattern_hit_counts": '
    return head, key + rest.split(key, 1)[1]


def sam_without_own_pg(data):
    return [ln for ln in data.split(b"\n") if not ln.startswith(b"@PG\tID:merkurio")]


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("bamsam")
    rnd = random.Random(5)
    kmers = [bytes(rnd.choice(b"ACGT") for _ in range(31)) for _ in range(200)]
    recs = make_records(rnd, kmers, 24000)
    write_bam(d / "in.bam", recs)
    (d / "k.txt").write_bytes(b"\n".join(kmers) + b"\n")
    return d, recs, kmers


def both(d, tag, extra, inp="in.bam", stdout=False):
    res = []
    for mode, flags in (("dev", []), ("host", ["--host-ingest"])):
        o, lg, js = d / f"{tag}_{mode}.sam", d / f"{tag}_{mode}.log", d / f"{tag}_{mode}.json"
        p = run(["tag", "-i", str(d / inp), "-f", str(d / "k.txt"), *([] if stdout else ["-o", str(o)]), "-l", str(lg), "-j", str(js), *extra, *flags])
        res.append((sam_without_own_pg(p.stdout if stdout else o.read_bytes()), log_body(lg), json_stable(js), p.stderr))
    return res


@pytest.mark.parametrize("extra", [[], ["-m"], ["-v"], ["--gpus", "2"], ["--window-mb", "1"], ["--window-mb", "1", "-m"],
                                   ["--window-mb", "1", "--gpus", "2", "-v"]], ids=lambda e: "_".join(e).replace("-", "") or "default")
def test_window_path_equals_host_path(job, extra):
    d, recs, _ = job
    dev, host = both(d, "o" + "".join(extra).replace("-", ""), extra)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    row = [ln for ln in dev[3].split(b"\n") if WINDOW_ROW in ln][0].split()
    assert row[1] == row[3], row
    if "--window-mb" in extra:  # (7 MB of BAM text: many windows, two in flight per device)
        assert int(row[1]) >= 5, row
        assert int(row[row.index(b"in") - 1][1:]) >= 2, row
    assert b"left to the host" not in dev[3]
    assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2]
    lines = [ln for ln in dev[0] if ln and not ln.startswith(b"@")]
    if "-m" in extra:
        assert 5000 < len(lines) < len(recs) and all(b"\tkm:Z:" in ln for ln in lines)
    elif "-v" in extra:
        assert len(recs) // 2 < len(lines) < len(recs) and all(ln.endswith(b"\tkm:Z:") or ln.endswith(b"\tkm:Z:OLD") for ln in lines)
    else:
        assert len(lines) == len(recs)


def test_stdout_equals_host_path(job):
    d, recs, _ = job
    dev, host = both(d, "so", ["-m", "--window-mb", "1"], stdout=True)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2]
    assert len([ln for ln in dev[0] if ln and not ln.startswith(b"@")]) > 5000


def test_gpus_2_equals_gpus_1(job):
    d, _, _ = job
    one = both(d, "g1", ["--window-mb", "1", "--gpus", "1"])[0]
    two = both(d, "g2", ["--window-mb", "1", "--gpus", "2"])[0]
    assert WINDOW_ROW in one[3] and WINDOW_ROW in two[3]
    assert one[0] == two[0] and one[1] == two[1] and one[2] == two[2]


def test_a_float_outside_the_rule_in_the_middle_gives_the_same_stream(job, tmp_path):
    """a record the device does not format but the host does (a float "%g" writes as 1e-05): the window path hands the input over at
    that window's first byte and the output stays continuous -- the device's lines first, then the host loop's"""
    d, recs, _ = job
    odd = list(recs)
    k = len(recs) // 2
    odd[k] = struct.pack("<i", struct.unpack_from("<i", odd[k], 0)[0] + 7) + odd[k][4:] + b"XEf" + struct.pack("<f", 1e-5)
    write_bam(tmp_path / "odd.bam", odd)
    res = []
    for flags in ([], ["--host-ingest"]):
        o = tmp_path / ("odd%d.sam" % len(res))
        p = run(["tag", "-i", str(tmp_path / "odd.bam"), "-f", str(d / "k.txt"), "-o", str(o), "--window-mb", "1", *flags])
        res.append((sam_without_own_pg(o.read_bytes()), p.stderr))
    assert WINDOW_ROW in res[0][1] and b"left to the host loop (a record the device does not format)" in res[0][1]
    row = [ln for ln in res[0][1].split(b"\n") if WINDOW_ROW in ln][0].split()
    assert 0 < int(row[1]) < int(row[3])  # some windows on the device, the rest on the host
    assert res[0][0] == res[1][0]
    lines = [ln for ln in res[0][0] if ln and not ln.startswith(b"@")]
    assert len(lines) == len(recs) and sum(b"\tXE:f:1e-05\t" in ln for ln in lines) == 1


def test_a_truncated_file_gets_the_host_error(job, tmp_path):
    d, recs, _ = job
    write_bam(tmp_path / "cut.bam", recs[:9000], cut=11)
    res = [run(["tag", "-i", str(tmp_path / "cut.bam"), "-f", str(d / "k.txt"), "-o", str(tmp_path / "cut.sam"), "--window-mb", "1", *flags], check=False)
           for flags in ([], ["--host-ingest"])]
    assert res[0].returncode == res[1].returncode != 0
    msg = [[ln for ln in p.stderr.split(b"\n") if ln and not ln.startswith(b"[timing]")] for p in res]
    assert msg[0] == msg[1] and any(b"truncated file" in ln for ln in msg[0])
    assert WINDOW_ROW in res[0].stderr and b"left to the host loop (unfinished record)" in res[0].stderr
