"""`merkurio extract --device-xz` on .xz inputs whose blocks are decoded on the device (mk_xz_inflate_device; the windows are ranges of
the text there) against `--host-codec` (liblzma inflates the file at load) and against the plain input: the kept records, the text
log and the JSON log byte for byte.  The [timing] row must name the path that ran: without that row these tests would pass on a
build that never leaves liblzma.  A file of one block (the spread rule), a BCJ file, a damaged file and a file of more compressed
bytes than --xz-window are liblzma's, which also words the error.  Without --device-xz an .xz input is liblzma's (the device path has
not been timed: it is opt-in)."""
import lzma
import os
import subprocess

import pytest

import xz_cases as cases
import xz_craft as craft
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu

PATTERN = "ACGTAC"  # (one read in ~14 of 150 bases holds it or its reverse complement)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
SPREAD = ["--xz-spread", "4"]  # (the files here have 12 even blocks: the default K would hand them back)


def blocks_xz(text, n, kind=4):
    """one stream of n blocks of about equal text (cut anywhere: in the middle of records)"""
    step = (len(text) + n - 1) // n
    return craft.stream([cases.real_block(text[k:k + step], kind) for k in range(0, len(text), step)], kind)[0]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("xzcli")
    fq, mate = cases.fastq(1600, seed=11), cases.fastq(1600, seed=12)
    with open(os.path.join(GOLDEN, "sample.fasta"), "rb") as f:
        fa = f.read()
    plain = {"single.fastq": fq, "mate.fastq": mate, "sample.fasta": fa, "oneblock.fastq": fq, "bcj.fastq": fq}
    files = {
        "single.fastq.xz": blocks_xz(fq, 12),
        "mate.fastq.xz": blocks_xz(mate, 12, kind=1),
        "sample.fasta.xz": blocks_xz(fa, 12),
        "oneblock.fastq.xz": lzma.compress(fq),
        "bcj.fastq.xz": lzma.compress(fq, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 6}]),
    }
    with open(os.path.join(GOLDEN, "sample.fasta.xz"), "rb") as f:  # the fixture as the xz tool wrote it: one block
        files["golden.fasta.xz"] = f.read()
    plain["golden.fasta"] = fa
    for name, blob in files.items():
        assert cases.liblzma_says(blob) == plain[name[:-3]], name
    files["damaged.fastq.xz"] = cases.flip(files["single.fastq.xz"], len(files["single.fastq.xz"]) * 4)  # one bit in the middle of the file
    assert cases.liblzma_says(files["damaged.fastq.xz"]) is None
    for name, blob in list(files.items()) + list(plain.items()):
        (d / name).write_bytes(blob)
    return d


def run(d, o, names, extra):
    o.mkdir(parents=True)
    ext = "fasta" if "fasta" in names[0] else "fastq"
    args = [BIN, "extract", "-i", str(d / names[0])] + (["-2", str(d / names[1])] if len(names) > 1 else [])
    args += ["-s", PATTERN, "-r", "-o", str(o / f"out.{ext}"), "-l", str(o / "x.log"), "-j", str(o / "x.json"), *extra]
    return subprocess.run(args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))


def same_outputs(a_dir, b_dir):
    fa, fb = sorted(os.listdir(a_dir)), sorted(os.listdir(b_dir))
    assert fa == fb, (fa, fb)
    for x in fa:
        if x == "x.log":
            assert log_body(a_dir / x) == log_body(b_dir / x)
        elif x == "x.json":
            assert json_stable(a_dir / x)[:2] == json_stable(b_dir / x)[:2]
        else:
            assert (a_dir / x).read_bytes() == (b_dir / x).read_bytes(), x


def compare(d, tmp_path, names, extra=SPREAD, device_takes=True, blocks=12):
    dev = run(d, tmp_path / "device", names, ["--device-xz", *extra])
    host = run(d, tmp_path / "host", names, ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    untimed = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert untimed(dev.stderr) == untimed(host.stderr)
    assert "xz on the device" not in host.stderr.decode(errors="replace")
    if dev.returncode != 0:
        assert all((tmp_path / "device" / f).stat().st_size == 0 for f in os.listdir(tmp_path / "device") if f.startswith("out"))
        return dev, err
    same_outputs(tmp_path / "device", tmp_path / "host")
    plain = run(d, tmp_path / "plain", [n[:-3] for n in names], [])
    assert plain.returncode == 0
    # the records (the logs name the input files; the derived output names differ by the input's extension: in sorted order)
    kept = lambda o: [(o / f).read_bytes() for f in sorted(os.listdir(o)) if f.startswith("out")]
    assert kept(tmp_path / "device") == kept(tmp_path / "plain") and len(kept(tmp_path / "plain")) == len(names)
    if not device_takes:
        assert "NOT taken by the device" in err and "xz on the device: " not in err, err
        return dev, err
    rows = [ln for ln in err.split("\n") if "xz on the device: " in ln]
    assert [ln.split("xz on the device: ")[1].split(" blocks,")[0] for ln in rows] == [str(blocks)] * len(names), err
    assert all(" 1 streams," in ln and "largest block" in ln and "upload" in ln and "decode" in ln and "check" in ln and "total" in ln for ln in rows), err
    return dev, err


def test_fastq_of_12_blocks(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz"])
    assert dev.returncode == 0
    kept = [f for f in os.listdir(tmp_path / "device") if f.startswith("out")]
    n = (tmp_path / "device" / kept[0]).read_bytes().count(b"\n")
    assert n % 4 == 0 and 50 < n // 4 < 1600  # some records, not all


def test_golden_fasta(inputs, tmp_path):
    assert compare(inputs, tmp_path, ["sample.fasta.xz"])[0].returncode == 0


def test_the_golden_fixture_as_the_xz_tool_wrote_it(inputs, tmp_path):
    """one block: tried under --xz-spread 1, handed back by the rule under the default"""
    assert compare(inputs, tmp_path / "k1", ["golden.fasta.xz"], extra=["--xz-spread", "1"], blocks=1)[0].returncode == 0
    dev, err = compare(inputs, tmp_path / "default", ["golden.fasta.xz"], extra=[], device_takes=False)
    assert dev.returncode == 0 and "status %d" % cases.XZ_SPREAD in err


def test_pair(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz", "mate.fastq.xz"])
    assert dev.returncode == 0 and err.count("xz on the device: ") == 2


def test_12_blocks_are_too_few_for_the_default_spread(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path / "none", ["single.fastq.xz"], extra=[], device_takes=False)
    assert dev.returncode == 0 and "status %d" % cases.XZ_SPREAD in err
    dev, err = compare(inputs, tmp_path / "zero", ["single.fastq.xz"], extra=["--xz-spread", "0"], device_takes=False)  # 0 = the default
    assert dev.returncode == 0 and "status %d" % cases.XZ_SPREAD in err


def test_a_single_block_is_handed_back_by_the_rule(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["oneblock.fastq.xz"], device_takes=False)
    assert dev.returncode == 0 and "status %d" % cases.XZ_SPREAD in err and "largest block %d text bytes" % len(cases.fastq(1600, seed=11)) in err


def test_a_bcj_file_is_handed_back(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["bcj.fastq.xz"], device_takes=False)
    assert dev.returncode == 0 and "status %d" % cases.XZ_FILTER in err


def test_a_flipped_bit_is_liblzmas_error(inputs, tmp_path):
    """the same message and exit status as --host-codec; the device hands the file back and says so"""
    dev, err = compare(inputs, tmp_path, ["damaged.fastq.xz"])
    assert dev.returncode != 0 and "Error while decompressing" in err
    assert "NOT taken by the device" in err and "xz on the device: " not in err


def test_a_file_above_the_window_is_liblzmas(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz"], SPREAD + ["--xz-window", "1"], device_takes=False)
    assert dev.returncode == 0 and "--xz-window" in err


def test_without_the_flag_liblzma_reads_the_file(inputs, tmp_path):
    off = run(inputs, tmp_path / "off", ["single.fastq.xz"], [])
    host = run(inputs, tmp_path / "host", ["single.fastq.xz"], ["--host-codec"])
    assert off.returncode == host.returncode == 0
    assert "xz on the device" not in off.stderr.decode(errors="replace") and "xz input" not in off.stderr.decode(errors="replace")
    same_outputs(tmp_path / "off", tmp_path / "host")
