"""`merkurio extract --device-zstd` on .zst inputs whose blocks are decoded on the device (mk_zstd_inflate_device; the windows are ranges
of the text there) against `--host-codec` (libzstd inflates the file at load) and against the plain input: the kept records, the text
log and the JSON log byte for byte.  The [timing] row must name the device path with the number of blocks that the host harness counts:
without that row these tests would pass on a build that never leaves libzstd.  A damaged file is handed back to libzstd, which words
the error, and the run ends as it does under --host-codec; so does a file of more compressed bytes than --zstd-window.  Without
--device-zstd a .zst input is libzstd's (the device path has not been timed: it is opt-in)."""
import os
import subprocess

import pytest

import zstd_cases as cases
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu

PATTERN = "ACGTAC"  # (one read in ~14 of 150 bases holds it or its reverse complement)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> blocks; the files lie in the returned directory.  FASTQ of a few blocks at levels 3 and 19, a file of two frames (the
    second starts in the middle of a record), the golden FASTA"""
    d = tmp_path_factory.mktemp("zscli")
    fq, mate = cases.fastq(1600, seed=11), cases.fastq(1600, seed=12)
    cut = fq.index(b"\n@read", len(fq) // 2) + 40
    with open(os.path.join(GOLDEN, "sample.fasta"), "rb") as f:
        fa = f.read()
    plain = {"single.fastq": fq, "mate.fastq": mate, "sample.fasta": fa}
    files = {
        "single.fastq.zst": cases.compress(fq, 3, True),
        "mate.fastq.zst": cases.compress(mate, 19, True),
        "l19.fastq.zst": cases.compress(fq, 19, False),
        "frames.fastq.zst": cases.compress(fq[:cut], 3, True) + cases.compress(fq[cut:], 19, True),
        "sample.fasta.zst": cases.compress(fa, 3, True),
    }
    damaged = cases.flip(files["single.fastq.zst"], len(files["single.fastq.zst"]) * 4)  # one bit in the middle of the file
    assert cases.libzstd_says(damaged) is None
    work = tmp_path_factory.mktemp("zsharness")
    exe = cases.build_harness(work, sanitize=False)
    blocks = {name: int(cases.run_harness(exe, work, blob)[0]["blocks"]) for name, blob in files.items()}
    assert blocks["single.fastq.zst"] >= 4 and blocks["frames.fastq.zst"] >= 4, blocks
    files["damaged.fastq.zst"] = damaged
    for name, blob in list(files.items()) + list(plain.items()):
        (d / name).write_bytes(blob)
    return d, blocks


def run(d, o, names, extra):
    o.mkdir(parents=True)
    ext = "fasta" if "fasta" in names[0] else "fastq"
    args = [BIN, "extract", "-i", str(d / names[0])] + (["-2", str(d / names[1])] if len(names) > 1 else [])
    args += ["-s", PATTERN, "-r", "-o", str(o / f"out.{ext}"), "-l", str(o / "x.log"), "-j", str(o / "x.json"), *extra]
    return subprocess.run(args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1"))


def same_outputs(a_dir, b_dir, names_differ=False):
    """kept records, text log and JSON log of two runs (the derived output names keep .zst: compared in sorted order)"""
    fa, fb = sorted(os.listdir(a_dir)), sorted(os.listdir(b_dir))
    assert len(fa) == len(fb) and (names_differ or fa == fb), (fa, fb)
    for x, y in zip(fa, fb):
        if x == "x.log":
            assert log_body(a_dir / x) == log_body(b_dir / y)
        elif x == "x.json":
            assert json_stable(a_dir / x)[:2] == json_stable(b_dir / y)[:2]
        else:
            assert (a_dir / x).read_bytes() == (b_dir / y).read_bytes(), (x, y)


def compare(inputs, tmp_path, names, extra=(), device_takes=True, against_plain=True):
    d, blocks = inputs
    dev = run(d, tmp_path / "device", names, ["--device-zstd", *extra])
    host = run(d, tmp_path / "host", names, ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    untimed = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert untimed(dev.stderr) == untimed(host.stderr)
    assert "zstd on the device" not in host.stderr.decode(errors="replace")
    if dev.returncode != 0:
        assert all((tmp_path / "device" / f).stat().st_size == 0 for f in os.listdir(tmp_path / "device") if f.startswith("out"))
        return dev, err
    same_outputs(tmp_path / "device", tmp_path / "host")
    if against_plain:
        plain = run(d, tmp_path / "plain", [n[:-4] for n in names], [])
        assert plain.returncode == 0
        # the records (the logs name the input files; the derived output names differ by the input's extension: in sorted order)
        kept = lambda o: [(o / f).read_bytes() for f in sorted(os.listdir(o)) if f.startswith("out")]
        assert kept(tmp_path / "device") == kept(tmp_path / "plain") and len(kept(tmp_path / "plain")) == len(names)
    if not device_takes:
        assert "NOT taken by the device" in err and "zstd on the device: " not in err, err
        return dev, err
    rows = [ln for ln in err.split("\n") if "zstd on the device: " in ln]
    assert [ln.split("zstd on the device: ")[1].split(" blocks,")[0] for ln in rows] == [str(blocks[n]) for n in names], err
    assert all("entropy decode" in ln and "cross-block rounds" in ln and "checksum" in ln for ln in rows), err
    return dev, err


def test_fastq_level_3(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"])
    assert dev.returncode == 0
    kept = [f for f in os.listdir(tmp_path / "device") if f.startswith("out")]
    n = (tmp_path / "device" / kept[0]).read_bytes().count(b"\n")
    assert n % 4 == 0 and 50 < n // 4 < 1600  # some records, not all


def test_fastq_level_19(inputs, tmp_path):
    assert compare(inputs, tmp_path, ["l19.fastq.zst"], against_plain=False)[0].returncode == 0


def test_golden_fasta(inputs, tmp_path):
    assert compare(inputs, tmp_path, ["sample.fasta.zst"])[0].returncode == 0


def test_pair(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst", "mate.fastq.zst"])
    assert dev.returncode == 0 and err.count("zstd on the device: ") == 2


def test_two_frames(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["frames.fastq.zst"], against_plain=False)
    assert dev.returncode == 0 and " 2 frames," in err
    d, _ = inputs
    one = run(d, tmp_path / "one", ["single.fastq.zst"], ["--host-codec"])
    assert one.returncode == 0
    for f in os.listdir(tmp_path / "device"):
        if f.startswith("out"):
            assert (tmp_path / "device" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f


def test_a_flipped_bit_is_libzstds_error(inputs, tmp_path):
    """the same message and exit status as --host-codec; the device hands the file back and says so"""
    dev, err = compare(inputs, tmp_path, ["damaged.fastq.zst"])
    assert dev.returncode != 0 and "Error while decompressing" in err
    assert "NOT taken by the device" in err and "zstd on the device: " not in err


def test_a_file_above_the_window_is_libzstds(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"], ["--zstd-window", "1"], device_takes=False, against_plain=False)
    assert dev.returncode == 0 and "--zstd-window" in err


def test_without_the_flag_libzstd_reads_the_file(inputs, tmp_path):
    d, _ = inputs
    off = run(d, tmp_path / "off", ["single.fastq.zst"], [])
    host = run(d, tmp_path / "host", ["single.fastq.zst"], ["--host-codec"])
    assert off.returncode == host.returncode == 0
    assert "zstd on the device" not in off.stderr.decode(errors="replace") and "zstd input" not in off.stderr.decode(errors="replace")
    same_outputs(tmp_path / "off", tmp_path / "host")
