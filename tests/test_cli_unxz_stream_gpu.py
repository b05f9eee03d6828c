"""`merkurio extract --xz-stream` on .xz inputs that are decoded on the device window by window (--xz-window 1 --xz-spread 1
--xz-text-cap <a few blocks>, mk_xz_stream_*) against the same command under `--host-codec` (liblzma inflates the file at load): the
kept records, the text log and the JSON log byte for byte.  The files hold ~530 KB of text in 12 blocks cut anywhere, so a record
crosses nearly every seam through the chained tails and heads.  The summary [timing] row must name the number of windows that the
host harness of the chain computes: without that check these tests would pass on a build that never streams."""
import os

import pytest

import xz_cases as cases
import xz_craft as craft
import xz_windows_cases as wc
from test_cli_gpu import log_body
from test_cli_unxz_gpu import GOLDEN, blocks_xz, run, same_outputs

pytestmark = pytest.mark.gpu

CAP = 100000  # text bytes per window: two blocks of the FASTQ files (~44 KB each)
FASTA_CAP = 500  # three blocks of the FASTA file (1858 bytes in 12 blocks)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (the directory of the files, windows(name): what the chain's host harness counts at the text cap)"""
    d = tmp_path_factory.mktemp("xzwin")
    fq, mate = cases.fastq(1600, seed=11), cases.fastq(1600, seed=12)
    with open(os.path.join(GOLDEN, "sample.fasta"), "rb") as f:
        fa = f.read()
    half = len(fq) // 2 + 77
    plain = {"single.fastq": fq, "mate.fastq": mate, "sample.fasta": fa, "streams.fastq": fq}
    files = {
        "single.fastq.xz": blocks_xz(fq, 12),
        "mate.fastq.xz": blocks_xz(mate, 12, kind=1),
        "sample.fasta.xz": blocks_xz(fa, 12),
        # three streams, one without blocks, padding between them, two check kinds; the seam between them inside a record
        "streams.fastq.xz": blocks_xz(fq[:half], 5) + b"\0" * 8 + craft.stream([], 4)[0] + blocks_xz(fq[half:], 6, kind=1) + b"\0" * 4,
    }
    for name, blob in files.items():
        assert cases.liblzma_says(blob) == plain[name[:-3]], name
    work = tmp_path_factory.mktemp("xzwin-harness")
    exe = wc.build_harness(work, sanitize=False)
    rows = wc.run_plan(exe, work, files["single.fastq.xz"])[1]
    late = rows[9]
    files["damaged.fastq.xz"] = cases.flip(files["single.fastq.xz"], (late[0] + late[1] // 2) * 8 + 3)  # one bit in the tenth block's payload
    assert cases.liblzma_says(files["damaged.fastq.xz"]) is None
    for name, blob in list(files.items()) + list(plain.items()):
        (d / name).write_bytes(blob)
    return d, lambda name, cap=CAP: wc.run_stream(exe, work, files[name], 0, cap)[0]


def stream_flags(cap=CAP):
    return ["--xz-stream", "--xz-window", "1", "--xz-spread", "1", "--xz-text-cap", str(cap)]


def compare(inputs, tmp_path, names, extra=(), streamed=True, cap=CAP):
    d, windows = inputs
    dev = run(d, tmp_path / "device", names, [*stream_flags(cap), *extra])
    host = run(d, tmp_path / "host", names, [*stream_flags(cap), "--host-codec", *extra])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    untimed = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert untimed(dev.stderr) == untimed(host.stderr)  # the same message
    assert "xz input" not in host.stderr.decode(errors="replace")
    if dev.returncode == 0:
        same_outputs(tmp_path / "device", tmp_path / "host")
    else:  # nothing written that --host-codec would not write
        assert sorted(os.listdir(tmp_path / "device")) == sorted(os.listdir(tmp_path / "host"))
        for f in sorted(os.listdir(tmp_path / "device")):  # both logs (and a kept records' file, were there one)
            a, b = tmp_path / "device" / f, tmp_path / "host" / f
            if f == "x.log":  # (its first four lines hold the time and the command line)
                assert log_body(a) == log_body(b) and len(a.read_bytes().split(b"\n", 4)) == 5
            else:
                assert a.read_bytes() == b.read_bytes(), f
    if streamed:
        for i, name in enumerate(names):
            want = windows(name, cap)
            assert want["state"] == "1" and int(want["windows"]) >= 2, want
            assert "xz input %d on the device, window by window: %s planned windows, %s windows, %s blocks, %s streams closed, largest block %s text bytes," % (
                i, want["planned"], want["windows"], want["blocks"], want["streams"], want["largest"]) in err, (want, err)
            rows = [ln for ln in err.split("\n") if "xz input %d on the device: window" % i in ln]
            assert len(rows) == int(want["windows"]), err
        assert err.count("handed back at -") == len(names) and "xz on the device: " not in err and "NOT taken" not in err, err
    return dev, err


def kept_files(o):
    return [o / f for f in sorted(os.listdir(o)) if f.startswith("out")]


def test_fastq_records_cross_every_seam(inputs, tmp_path):
    d, _ = inputs
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz"])
    assert dev.returncode == 0
    kept = kept_files(tmp_path / "device")[0].read_bytes()
    assert kept.count(b"\n") % 4 == 0 and 50 < kept.count(b"\n") // 4 < 1600  # some records, not all
    text = (d / "single.fastq").read_bytes()
    sizes = [int(ln.split("taken, ")[1].split(" text bytes")[0]) for ln in err.split("\n") if "xz input 0 on the device: window" in ln]
    assert sum(sizes) == len(text) and len(sizes) >= 4
    seams, at = 0, 0
    for s in sizes[:-1]:
        at += s
        seams += text[at - 1:at] != b"\n" or text[at:at + 1] != b"@"
    assert seams >= 3, sizes


def test_fasta(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["sample.fasta.xz"], cap=FASTA_CAP)
    assert dev.returncode == 0 and len(kept_files(tmp_path / "device")) == 1


def test_pair_both_streamed_side_by_side(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz", "mate.fastq.xz"])
    assert dev.returncode == 0 and len(kept_files(tmp_path / "device")) == 2


def test_invert_match(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.xz"], extra=["-v"])
    assert dev.returncode == 0


def test_streams_padding_and_a_stream_without_blocks(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["streams.fastq.xz"])
    assert dev.returncode == 0 and " 3 streams closed," in err and " 11 blocks," in err, err


def test_a_late_damaged_block_is_liblzmas_error(inputs, tmp_path):
    """the windows in front of the damage are taken, then the stream hands the file back and liblzma words the error: the same
    message and exit status as --host-codec"""
    dev, err = compare(inputs, tmp_path, ["damaged.fastq.xz"], streamed=False)
    assert dev.returncode != 0
    assert err.count("xz input 0 on the device: window") == 4 and "liblzma reads on" in err, err  # (blocks 0 .. 7 in four windows; the tenth is in the fifth)


def test_without_the_flag_a_larger_file_is_liblzmas(inputs, tmp_path):
    d, _ = inputs
    dev = run(d, tmp_path / "device", ["single.fastq.xz"], ["--device-xz", "--xz-window", "1", "--xz-spread", "1"])
    host = run(d, tmp_path / "host", ["single.fastq.xz"], ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    assert dev.returncode == 0 and host.returncode == 0
    assert "more compressed bytes than --xz-window" in err and "window by window" not in err, err
    same_outputs(tmp_path / "device", tmp_path / "host")


def test_the_timing_rows(inputs, tmp_path):
    d, windows = inputs
    dev = run(d, tmp_path / "device", ["single.fastq.xz"], stream_flags())
    err = dev.stderr.decode(errors="replace")
    want = windows("single.fastq.xz")
    rows = [ln for ln in err.split("\n") if "xz input 0 on the device: window" in ln]
    assert dev.returncode == 0 and len(rows) == int(want["windows"]) == 6, err
    assert all("taken" in ln and "text bytes" in ln and "compressed bytes consumed" in ln for ln in rows)
    summary = [ln for ln in err.split("\n") if "xz input 0 on the device, window by window:" in ln]
    assert len(summary) == 1 and "6 planned windows, 6 windows, 12 blocks, 1 streams closed, largest block" in summary[0] and "upload" in summary[0], summary
