"""`merkurio extract` on .bz2 inputs that are decoded on the device window by window (--bzip2-window 65536, mk_bzip2_stream_*) against
`--host-codec` (libbz2 inflates the file at load): the kept records, the text log and the JSON log byte for byte.  The files hold 1.6 -
2.6 MB of text in level-1 blocks, 0.4 - 0.7 MB of compressed bytes: six bzip2 windows at least, records cross the windows' cuts
through the chained tails and heads.  The [timing] rows must name the stream: without them these tests would pass on a build that
never leaves libbz2 or the one-shot call."""
import bz2
import gzip
import os
import random
import subprocess

import pytest

import bzip2_cases as cases
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu

WINDOW = 65536
PATTERN = "ACGTAC"  # (one read in ~14 of 150 bases holds it or its reverse complement)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


def fasta_with_broken_hits(n, seed):
    """records of 70-base lines; every fifth one holds the pattern across a line break"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        seq = rng.choices("ACGT", k=rng.randrange(200, 900))
        if i % 5 == 0:
            seq[67:73] = PATTERN
        seq = "".join(seq)
        out.append(">contig%d len=%d\n%s\n" % (i, len(seq), "\n".join(seq[p:p + 70] for p in range(0, len(seq), 70))))
    return "".join(out).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bzwin")
    fq, mate = cases.fastq(5000, seed=21), cases.fastq(5000, seed=22)
    files = {
        "single.fastq.bz2": bz2.compress(fq, 1),
        "mate.fastq.bz2": bz2.compress(mate, 1),
        "contigs.fasta.bz2": bz2.compress(fasta_with_broken_hits(4000, 6), 1),
        # pbzip2's output: a stream per 100 000 bytes of input, cut wherever that falls
        "pbzip2.fastq.bz2": b"".join(bz2.compress(fq[p:p + 100000], 1) for p in range(0, len(fq), 100000)),
        "crlf.fastq.bz2": bz2.compress(fq.replace(b"\n", b"\r\n"), 1),
        "unterminated.fastq.bz2": bz2.compress(fq[:-1], 1),
        "small.fastq.bz2": bz2.compress(cases.fastq(300, seed=23), 1),
    }
    damaged = bytearray(files["single.fastq.bz2"])
    damaged[len(damaged) * 9 // 10] ^= 0x10  # one bit of a late block's symbols
    assert cases.libbz2_says(bytes(damaged)) is None
    files["damaged.fastq.bz2"] = bytes(damaged)
    for name, blob in files.items():
        (d / name).write_bytes(blob)
        assert name == "small.fastq.bz2" or len(blob) > 5 * WINDOW, (name, len(blob))
    assert len(files["small.fastq.bz2"]) <= WINDOW
    return d


def compare(inputs, tmp_path, names, extra=(), streamed=True):
    run_dir = tmp_path / "runs"
    run_dir.mkdir()

    def go(tag, codec):
        o = run_dir / tag
        o.mkdir()
        ext = "fasta" if "fasta" in names[0] else "fastq"
        args = [BIN, "extract", "-i", str(inputs / names[0])] + (["-2", str(inputs / names[1])] if len(names) > 1 else [])
        args += ["-s", PATTERN, "-r", "-o", str(o / f"out.{ext}"), "-l", str(o / "x.log"), "-j", str(o / "x.json"), *extra, *codec]
        return subprocess.run(args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1")), o
    dev, d_dir = go("device", ["--bzip2-window", str(WINDOW)])
    host, h_dir = go("host", ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    plain = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert plain(dev.stderr) == plain(host.stderr)  # the same message
    assert "bzip2 input" not in host.stderr.decode(errors="replace")
    if dev.returncode != 0:
        return dev, err, d_dir
    assert sorted(os.listdir(d_dir)) == sorted(os.listdir(h_dir))
    for f in sorted(os.listdir(d_dir)):
        a, b = (d_dir / f).read_bytes(), (h_dir / f).read_bytes()
        if f == "x.log":
            assert log_body(d_dir / f) == log_body(h_dir / f)
        elif f == "x.json":
            assert json_stable(d_dir / f)[:2] == json_stable(h_dir / f)[:2]
        elif f.endswith(".gz"):
            assert gzip.decompress(a) == gzip.decompress(b) and len(gzip.decompress(a)) > 0, f
        else:
            assert a == b, f
    if streamed:
        for i in range(len(names)):
            assert err.count("bzip2 input %d on the device: window" % i) >= 5, err
            assert "bzip2 input %d on the device, window by window:" % i in err, err
        assert err.count("handed back at -") == len(names) and "bzip2 on the device: " not in err, err  # to the files' ends, never the one-shot call
    return dev, err, d_dir


def test_single_fastq(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2"])
    assert dev.returncode == 0
    kept = (o / "out.fastq").read_bytes()
    assert kept.count(b"\n") % 4 == 0 and 200 < kept.count(b"\n") // 4 < 5000  # some records, not all


def test_fasta_with_hits_across_line_breaks(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["contigs.fasta.bz2"])
    assert dev.returncode == 0 and (o / "out.fasta").read_bytes().count(b">") >= 800


def test_pair_both_streamed_side_by_side(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2", "mate.fastq.bz2"])
    assert dev.returncode == 0


def test_pbzip2_style_streams(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["pbzip2.fastq.bz2"])
    streams = -(-len(cases.fastq(5000, seed=21)) // 100000)
    assert dev.returncode == 0 and streams >= 16 and "%d streams closed" % streams in err, err
    # the same text as the one-stream file: the same records are kept, and some record spans a window seam whatever the cuts are
    (tmp_path / "one").mkdir()
    one = compare(inputs, tmp_path / "one", ["single.fastq.bz2"])[2]
    assert (o / "out.fastq").read_bytes() == (one / "out.fastq").read_bytes()


def test_crlf_records(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["crlf.fastq.bz2"])
    assert dev.returncode == 0 and (o / "out.fastq").stat().st_size > 0


def test_an_unterminated_last_record(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["unterminated.fastq.bz2"])
    assert dev.returncode == 0


def test_records_span_the_windows_seams(inputs, tmp_path):
    """a window's text is whole blocks of ~100 000 bytes and a record is ~330: every seam but one in 330 cuts a record.  The windows'
    sizes say so, and the output above is --host-codec's all the same"""
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2"], ["-v"])
    assert dev.returncode == 0
    text = bz2.decompress((inputs / "single.fastq.bz2").read_bytes())
    sizes = [int(ln.split("taken, ")[1].split(" text bytes")[0]) for ln in err.split("\n") if "bzip2 input 0 on the device: window" in ln]
    assert sum(sizes) == len(text) and len(sizes) >= 5
    seams, at = 0, 0
    for s in sizes[:-1]:
        at += s
        seams += text[at - 1:at] != b"\n" or text[at:at + 1] != b"@"
    assert seams >= 3, sizes


def test_bgzf_output(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2"], ["-z"])
    assert dev.returncode == 0 and (o / "out.fastq.gz").exists()


def test_damage_in_a_late_block_is_libbz2s_error(inputs, tmp_path):
    """the windows in front of the damage are taken, then the stream hands the file back and libbz2 words the error: the same message
    and exit status as --host-codec"""
    dev, err, o = compare(inputs, tmp_path, ["damaged.fastq.bz2"], streamed=False)
    assert dev.returncode != 0 and "Error while decompressing" in err
    assert "bzip2 input 0 on the device: window" in err and "libbz2 reads on" in err, err


def test_a_file_of_one_window_takes_the_one_shot_path(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["small.fastq.bz2"], streamed=False)
    assert dev.returncode == 0
    assert "bzip2 on the device: " in err and "block decode" in err and "window by window" not in err and "bzip2 input 0 on the device: window" not in err, err
