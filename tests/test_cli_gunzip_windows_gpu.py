"""`merkurio extract` on gzip inputs that are inflated on the device window by window (--gzip-window 262144, mk_gzip_stream_*)
against `--host-codec` (zlib reads the file): the output, the text log and the JSON log byte for byte.  The files hold 0.4 - 1.5 MB
of compressed bytes, 2 to 6 gzip windows; records cross the windows' cuts through the chained tails and heads."""
import gzip
import os
import random
import subprocess

import pytest

import gunzip_members_cases as gm
import gunzip_windows_cases as gw
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu

WINDOW = 262144
PATTERN = "ACGTAC"  # (one read in ~20 of 150 bases holds it or its reverse complement)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


def long_fasta():
    """small records around one of 3 MB of sequence: ~0.9 MB compressed, more than three windows"""
    rnd = random.Random(21)
    small = lambda k: b"".join(b">r%d\n%s\n" % (k * 100 + j, "".join(rnd.choices("ACGT", k=200)).encode()) for j in range(300))
    seq = "".join(rnd.choices("ACGT", k=3_000_000))
    big = ">huge\n" + "\n".join(seq[p:p + 80] for p in range(0, len(seq), 80)) + "\n"
    return small(1) + big.encode() + small(2)


def planted_fastq():
    """a FASTQ of one member whose middle is a stored block of five records with a gzip header's bytes in their names: more false
    member starts in one window than the stream drops -- it hands the file back there, zlib reads on"""
    plant = b"".join(b"@p%d \x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03 x\n%s\n+\n%s\n" % (k, b"ACGTACGT" * 10, b"F" * 80) for k in range(5))
    return gw.planted_headers([gm.fastq(4000, 31), gm.fastq(3000, 32)], plant, {0})[0]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzwin")
    files = {
        "single.fastq.gz": gm.member(gm.fastq(5000, 11)),
        "mate.fastq.gz": gm.member(gm.fastq(5000, 12)),
        "long.fasta.gz": gm.member(long_fasta()),
        "members.fastq.gz": gm.member(gm.fastq(2500, 13)) + gm.member(b"") + gm.member(gm.fastq(300, 14)) + gm.member(gm.fastq(2500, 15)),
        "planted.fastq.gz": planted_fastq(),
        "small.fastq.gz": gm.member(gm.fastq(300, 16)),
    }
    damaged = bytearray(files["single.fastq.gz"])
    damaged[len(damaged) // 2] ^= 0x10
    files["damaged.fastq.gz"] = bytes(damaged)
    for name, blob in files.items():
        (d / name).write_bytes(blob)
    for name in ("single.fastq.gz", "mate.fastq.gz", "long.fasta.gz", "members.fastq.gz", "planted.fastq.gz"):
        assert len(files[name]) > WINDOW, name
        assert gw.zlib_prefix(files[name])[1], name  # (zlib reads them to the end: the expectation is zlib's)
    assert len(files["small.fastq.gz"]) <= WINDOW
    return d


def json_parts(path):
    """json_stable's two texts; for a log whose record names are no UTF-8 (the planted headers), the same two cuts without the parse"""
    try:
        return json_stable(path)[:2]
    except UnicodeDecodeError:
        t = open(path, "rb").read()
        head, rest = t.split(b'  "meta_information": ', 1)
        key = b'  "pattern_hit_counts": '
        return head, key + rest.split(key, 1)[1]


def compare(inputs, tmp_path, names, extra=(), streamed=True):
    run_dir = tmp_path / "runs"
    run_dir.mkdir()
    def go(tag, codec):
        o = run_dir / tag
        o.mkdir()
        ext = "fasta" if "fasta" in names[0] else "fastq"
        args = [BIN, "extract", "-i", str(inputs / names[0])] + (["-2", str(inputs / names[1])] if len(names) > 1 else [])
        args += ["-s", PATTERN, "-r", "-o", str(o / f"out.{ext}"), "-l", str(o / "x.log"), "-j", str(o / "x.json"), *extra, *codec]
        p = subprocess.run(args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))
        return p, o
    dev, d_dir = go("device", ["--gzip-window", str(WINDOW)])
    host, h_dir = go("host", ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    plain = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert plain(dev.stderr) == plain(host.stderr)
    assert sorted(os.listdir(d_dir)) == sorted(os.listdir(h_dir))
    for f in sorted(os.listdir(d_dir)):
        a, b = (d_dir / f).read_bytes(), (h_dir / f).read_bytes()
        if dev.returncode != 0:
            if f.startswith("out"):
                assert a == b, f  # the same records written in front of the error
        elif f == "x.log":
            assert log_body(d_dir / f) == log_body(h_dir / f)
        elif f == "x.json":
            assert json_parts(d_dir / f) == json_parts(h_dir / f)
        elif f.endswith(".gz"):
            assert gzip.decompress(a) == gzip.decompress(b), f
            assert len(gzip.decompress(a)) > 0
        else:
            assert a == b, f
    if streamed:
        rows = [ln for ln in err.split("\n") if "window by window" in ln or ("on the device: window" in ln and "taken" in ln)]
        assert any("window by window:" in ln and "windows" in ln for ln in rows), err
    return dev, err, d_dir


def test_single_fastq(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["single.fastq.gz"])
    assert dev.returncode == 0 and (d / "out.fastq").stat().st_size > 0
    assert err.count("on the device: window") >= 2 and "handed back at -" in err  # several windows, to the file's end


def test_paired_fastq(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["single.fastq.gz", "mate.fastq.gz"])
    assert dev.returncode == 0
    assert "gzip input 0 on the device, window by window:" in err and "gzip input 1 on the device, window by window:" in err
    assert err.count("handed back at -") == 2


def test_fasta_record_longer_than_three_windows(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["long.fasta.gz"])
    assert dev.returncode == 0 and err.count("on the device: window") >= 4 and "handed back at -" in err


def test_inverted(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["single.fastq.gz"], ["-v"])
    assert dev.returncode == 0 and "handed back at -" in err


def test_bgzf_output(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["single.fastq.gz"], ["-z"])
    assert dev.returncode == 0 and (d / "out.fastq.gz").exists() and "handed back at -" in err


def test_two_gpus(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["single.fastq.gz"], ["--gpus", "2"])
    assert dev.returncode == 0 and "handed back at -" in err


def test_multi_member(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["members.fastq.gz"])
    assert dev.returncode == 0 and "4 members proved" in err and "handed back at -" in err


def test_damaged_in_the_middle(inputs, tmp_path):
    """the same records in front of the error, the same error text, the same exit status as --host-codec"""
    dev, err, d = compare(inputs, tmp_path, ["damaged.fastq.gz"], streamed=False)
    assert dev.returncode != 0 and "Error while decompressing" in err


def test_handed_back_in_the_middle(inputs, tmp_path):
    """a file zlib reads to its end and the stream hands back in the middle (state 2): zlib skips what the windows used and reads on"""
    dev, err, d = compare(inputs, tmp_path, ["planted.fastq.gz"])
    assert dev.returncode == 0
    assert "zlib reads on" in err and "handed back at 0 text" not in err, err


def test_one_window_takes_the_one_shot_path(inputs, tmp_path):
    dev, err, d = compare(inputs, tmp_path, ["small.fastq.gz"], streamed=False)
    assert dev.returncode == 0
    assert "gzip input 0 on the device: taken" in err and "window by window" not in err
