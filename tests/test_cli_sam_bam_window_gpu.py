"""`merkurio tag` with plain SAM input and BAM output encodes a window's kept lines as BAM records on the device
(mk_tag_sam_bam_window, cli/tag_windows.cpp: tag_sam_bam_windows_on_device) unless --host-ingest or --host-codec asks for the host
loop: both must give the same BAM -- the inflated stream byte for byte apart from the command line in the writer's own @PG header
line --, the same text log body, the same stable parts of the JSON log, and the same errors.  Under MERKURIO_TIMING=1 the window path
prints a row of its own, which is how these tests know which path ran."""
import gzip
import os
import random
import struct
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
GOLDEN = os.path.join(ROOT, "tests", "golden")
WINDOW_ROW = b"SAM text -> BAM windows on the device"


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


def bam_parts(path):
    """the inflated stream of a BAM file -> (header lines without the writer's own @PG line, reference dictionary, record bytes)"""
    raw = open(path, "rb").read()
    assert raw.endswith(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
    t = gzip.decompress(raw)
    assert t[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", t, 4)[0]
    text = t[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", t, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", t, at)[0]
        refs.append((t[at + 4:at + 4 + l_name], struct.unpack_from("<i", t, at + 4 + l_name)[0]))
        at += 8 + l_name
    return [ln for ln in text.split(b"\n") if not ln.startswith(b"@PG\tID:merkurio")], refs, t[at:]


def records(blob):
    """record bytes -> [(name, sequence, optional-field bytes)]"""
    out, at = [], 0
    while at < len(blob):
        size = struct.unpack_from("<i", blob, at)[0]
        r = blob[at + 4:at + 4 + size]
        l_name, n_cig, l_seq = r[8], struct.unpack_from("<H", r, 12)[0], struct.unpack_from("<i", r, 16)[0]
        p = 32 + l_name + 4 * n_cig
        seq = "".join("=ACMGRSVTWYHKDBN"[(r[p + k // 2] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(l_seq))
        out.append((r[32:32 + l_name - 1], seq.encode(), r[p + (l_seq + 1) // 2 + l_seq:]))
        at += 4 + size
    assert at == len(blob)
    return out


def log_body(path):
    return open(path, "rb").read().split(b"\n", 4)[4]


def json_stable(path):
    t = open(path, "rb").read()
    head, rest = t.split(b'  "meta_information": ', 1)
    key = b'  "pattern_hit_counts": '
    return head, key + rest.split(key, 1)[1]


def make_lines(rnd, kmers, n):
    lines = []
    for i in range(n):
        L = rnd.choice((50, 150, 151))
        s = "".join(rnd.choice("ACGTacgt" if i % 50 == 0 else "ACGTN") for _ in range(L))
        if i % 4 == 0:
            k = rnd.choice(kmers)
            o = rnd.randrange(len(s) - 31)
            s = s[:o] + k + s[o + 31:]
        q = "*" if i % 17 == 0 else "".join(chr(rnd.randrange(33, 127)) for _ in range(L))
        if i % 5 == 0:
            fixed = f"r{i}\t4\t*\t0\t0\t*\t*\t0\t0"
        else:
            fixed = f"r{i}\t{rnd.choice((99, 147, 0, 16))}\t{rnd.choice(('1', '2', 'MT', 'nowhere'))}\t{rnd.randrange(1, 10 ** 8)}\t{rnd.randrange(61)}\t" \
                    f"{rnd.randrange(1, 40)}S{L}M3D2I\t{rnd.choice(('=', '*', '2'))}\t{rnd.randrange(10 ** 8)}\t{rnd.randrange(-500, 500)}"
        aux = ["NM:i:%d" % rnd.randrange(-3, 70000), "de:f:0.0%d" % rnd.randrange(1000), "RG:Z:g%d" % (i % 3), "XB:B:s,1,-2,3", "XE:f:1e-05", "XA:A:c"][:i % 7]
        if i % 1000 == 0:
            aux.append("km:Z:OLD")
        lines.append("\t".join([fixed, s, q] + aux) + "\n")
    return lines


HEADER = "@HD\tVN:1.6\n@SQ\tSN:1\tLN:100000000\n@SQ\tSN:2\tLN:100000000\n@SQ\tSN:MT\tLN:16569\n@SQ\tSN:2\tLN:5\n"


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("sambam")
    rnd = random.Random(5)
    kmers = ["".join(rnd.choice("ACGT") for _ in range(31)) for _ in range(200)]
    lines = make_lines(rnd, kmers, 30000)
    (d / "in.sam").write_text(HEADER + "".join(lines))
    (d / "k.txt").write_text("\n".join(kmers) + "\n")
    return d, lines


def both(d, tag, extra, inp="in.sam"):
    res = []
    for mode, flags in (("dev", []), ("host", ["--host-ingest"])):
        o, lg, js = d / f"{tag}_{mode}.bam", d / f"{tag}_{mode}.log", d / f"{tag}_{mode}.json"
        p = run(["tag", "-i", str(d / inp), "-f", str(d / "k.txt"), "-o", str(o), "-l", str(lg), "-j", str(js), *extra, *flags])
        res.append((bam_parts(o), log_body(lg), json_stable(js), p.stderr))
    return res


@pytest.mark.parametrize("extra", [[], ["-m"], ["-v"], ["--gpus", "2"], ["--window-mb", "1"], ["--window-mb", "1", "-m"],
                                   ["--window-mb", "1", "--gpus", "2", "-v"]], ids=lambda e: "_".join(e).replace("-", "") or "default")
def test_window_path_equals_host_path(job, extra):
    d, lines = job
    dev, host = both(d, "o" + "".join(extra).replace("-", ""), extra)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    if "--window-mb" in extra:  # (9 MB of text: many windows)
        row = [ln for ln in dev[3].split(b"\n") if WINDOW_ROW in ln][0].split()
        assert row[1] == row[3] and int(row[1]) >= 5, row
    assert b"left to the host loop" not in dev[3]
    assert dev[0][0] == host[0][0] and dev[0][1] == host[0][1] == [(b"1\0", 100000000), (b"2\0", 100000000), (b"MT\0", 16569), (b"2\0", 5)]
    assert dev[0][2] == host[0][2]
    assert dev[1] == host[1] and dev[2] == host[2]
    recs = records(dev[0][2])
    if "-m" in extra:
        assert 7000 < len(recs) < 30000 and all(b"kmZ" in r[2] for r in recs)
    elif "-v" in extra:
        assert 15000 < len(recs) < 30000 and all(r[2].endswith(b"kmZ\0") or r[2].endswith(b"kmZOLD\0") for r in recs)
    else:
        assert len(recs) == 30000


def test_host_codec_takes_the_host_loop(job):
    d, _ = job
    p = run(["tag", "-i", str(d / "in.sam"), "-f", str(d / "k.txt"), "-o", str(d / "hc.bam"), "--host-codec", "-m"])
    assert WINDOW_ROW not in p.stderr
    q = run(["tag", "-i", str(d / "in.sam"), "-f", str(d / "k.txt"), "-o", str(d / "hc_dev.bam"), "-m"])
    assert WINDOW_ROW in q.stderr
    assert bam_parts(d / "hc.bam")[2] == bam_parts(d / "hc_dev.bam")[2]


@pytest.mark.parametrize("field", ["XF:f:1e-45", "XF:f:inf", "NM:i: 7"], ids=["float_outside_the_rule", "inf", "blank_in_integer"])
def test_a_refusing_line_in_the_middle_gives_the_same_stream(job, tmp_path, field):
    """a line the device does not encode but the host does (strtof / strtoll take it): the window path hands the input over at that
    window's first byte and the stream stays continuous -- members first, then the host loop's pieces"""
    d, lines = job
    odd = list(lines)
    k = len(lines) // 2
    odd[k] = odd[k].rstrip("\n") + "\t" + field + "\n"
    (tmp_path / "odd.sam").write_text(HEADER + "".join(odd))
    res = []
    for flags in ([], ["--host-ingest"]):
        o = tmp_path / ("odd%d.bam" % len(res))
        p = run(["tag", "-i", str(tmp_path / "odd.sam"), "-f", str(d / "k.txt"), "-o", str(o), "--window-mb", "1", *flags])
        res.append((bam_parts(o), p.stderr))
    assert WINDOW_ROW in res[0][1] and b"left to the host loop (a record the device does not encode)" in res[0][1]
    row = [ln for ln in res[0][1].split(b"\n") if WINDOW_ROW in ln][0].split()
    assert 0 < int(row[1]) < int(row[3])  # some windows on the device, the rest on the host
    assert res[0][0] == res[1][0] and len(records(res[0][0][2])) == 30000


def test_a_malformed_line_gets_the_host_error(job, tmp_path):
    d, lines = job
    for bad_cigar in (False, True):
        odd = list(lines)
        k = len(lines) // 2 + 1
        f = odd[k].rstrip("\n").split("\t")
        if bad_cigar:
            f[5] = "10Q"
        else:
            f[10] = f[10] + "I" if f[10] != "*" else "II"
        odd[k] = "\t".join(f) + "\n"
        (tmp_path / "bad.sam").write_text(HEADER + "".join(odd))
        res = [run(["tag", "-i", str(tmp_path / "bad.sam"), "-f", str(d / "k.txt"), "-o", str(tmp_path / "bad.bam"), "--window-mb", "1", *flags], check=False)
               for flags in ([], ["--host-ingest"])]
        assert res[0].returncode == res[1].returncode != 0
        msg = [[ln for ln in p.stderr.split(b"\n") if ln and not ln.startswith(b"[timing]")] for p in res]
        assert msg[0] == msg[1] and any((b"bad CIGAR" if bad_cigar else b"SEQ and QUAL lengths differ") in ln for ln in msg[0])
        assert b"left to the host loop" in res[0].stderr


def test_reference_fixtures(tmp_path):
    """the reference's own fixtures: simple.sam -> BAM, read back, gives the names, sequences and km values of its goldens"""
    fx = os.path.join(GOLDEN, "fixtures")

    def golden(name):
        out = []
        for ln in open(os.path.join(fx, "tag", name), "rb").read().split(b"\n"):
            if ln and ln[:1] != b"@":
                f = ln.split(b"\t")
                out.append((f[0], f[9], [x[5:] for x in f[11:] if x.startswith(b"km:Z:")][-1]))
        return out

    for flags, name in ((["-m"], "simple.extracted.sam"), (["-v"], "simple-inv.extracted.sam")):
        o = tmp_path / (name + ".bam")
        p = run(["tag", "-i", os.path.join(fx, "input", "simple.sam"), "-s", "CTC", "-r", "-o", str(o), *flags])
        assert WINDOW_ROW in p.stderr and b"left to the host loop" not in p.stderr
        head, refs, blob = bam_parts(o)
        assert refs == [(b"1\0", 100000)]
        got = [(nm, seq, aux[aux.rindex(b"kmZ") + 3:-1]) for (nm, seq, aux) in records(blob)]
        assert got == golden(name)
