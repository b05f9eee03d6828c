"""`merkurio extract --zstd-stream` on .zst inputs that are decoded on the device window by window (--zstd-window <small>,
mk_zstd_stream_*) against `--host-codec` (libzstd inflates the file at load) and against the plain input: the kept records, the text
log and the JSON log byte for byte.  The files hold ~530 KB of text in blocks of 128 KiB: at --zstd-window 1 a window per block, at
--zstd-window 100000 two or three of them, and a record of ~330 bytes crosses nearly every seam through the chained tails and heads.
The summary [timing] row must name the number of windows that the host harness of the chain computes: without that check these tests
would pass on a build that never streams."""
import gzip
import os

import pytest

import zstd_cases as cases
import zstd_windows_cases as wc
from test_cli_gpu import json_stable, log_body
from test_cli_unzstd_gpu import GOLDEN, run, same_outputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """-> (the directory of the files, windows(name, window): what the chain's host harness counts)"""
    d = tmp_path_factory.mktemp("zswin")
    fq, mate = cases.fastq(1600, seed=11), cases.fastq(1600, seed=12)
    cut = fq.index(b"\n@read", len(fq) // 2) + 40
    with open(os.path.join(GOLDEN, "sample.fasta"), "rb") as f:
        fa = f.read()
    plain = {"single.fastq": fq, "mate.fastq": mate, "sample.fasta": fa, "frames.fastq": fq, "small.fastq": fq[:fq.index(b"\n@read", 30000) + 1]}
    files = {
        "single.fastq.zst": cases.compress(fq, 3, True),
        "mate.fastq.zst": cases.compress(mate, 19, True),
        "frames.fastq.zst": cases.compress(fq[:cut], 3, True) + cases.compress(fq[cut:], 19, True),
        "sample.fasta.zst": cases.compress(fa, 3, True),
        "small.fastq.zst": cases.compress(plain["small.fastq"], 3, True),
    }
    single = files["single.fastq.zst"]
    files["damaged.fastq.zst"] = cases.flip(single, (len(single) - 40) * 8 + 3)  # one bit of the last block's sequences
    assert cases.libzstd_says(files["damaged.fastq.zst"]) is None
    for name, blob in list(files.items()) + list(plain.items()):
        (d / name).write_bytes(blob)
    work = tmp_path_factory.mktemp("zswin-harness")
    exe = wc.build_harness(work, sanitize=False)
    return d, lambda name, window: wc.run_harness(exe, work, files[name], "stream", window, 0)[0]


def kept_files(o):
    """the kept records' files (their names derive from the inputs' and keep .zst)"""
    return [o / f for f in sorted(os.listdir(o)) if f.startswith("out")]


def compare(inputs, tmp_path, names, window=1, extra=(), streamed=True, against_plain=True, min_windows=2):
    d, windows = inputs
    dev = run(d, tmp_path / "device", names, ["--zstd-stream", "--zstd-window", str(window), *extra])
    host = run(d, tmp_path / "host", names, ["--host-codec", *extra])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    untimed = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert untimed(dev.stderr) == untimed(host.stderr)  # the same message
    assert "zstd input" not in host.stderr.decode(errors="replace")
    if dev.returncode != 0:
        return dev, err
    if any(f.endswith(".gz") for f in os.listdir(tmp_path / "device")):
        assert sorted(os.listdir(tmp_path / "device")) == sorted(os.listdir(tmp_path / "host"))
        for f in sorted(os.listdir(tmp_path / "device")):
            a, b = tmp_path / "device" / f, tmp_path / "host" / f
            if f == "x.log":
                assert log_body(a) == log_body(b)
            elif f == "x.json":
                assert json_stable(a)[:2] == json_stable(b)[:2]
            else:
                assert gzip.decompress(a.read_bytes()) == gzip.decompress(b.read_bytes()) and len(gzip.decompress(a.read_bytes())) > 0, f
    else:
        same_outputs(tmp_path / "device", tmp_path / "host")
        if against_plain:
            plain = run(d, tmp_path / "plain", [n[:-4] for n in names], [])
            assert plain.returncode == 0
            kept = lambda o: [(o / f).read_bytes() for f in sorted(os.listdir(o)) if f.startswith("out")]
            assert kept(tmp_path / "device") == kept(tmp_path / "plain") and len(kept(tmp_path / "plain")) == len(names)
    if streamed:
        for i, name in enumerate(names):
            want = windows(name, window)
            assert want["state"] == "1" and int(want["windows"]) >= min_windows, want
            assert "zstd input %d on the device, window by window: %s windows, %s frames closed, %s blocks, %s rounds," % (
                i, want["windows"], want["frames"], want["blocks"], want["rounds"]) in err, (want, err)
            rows = [ln for ln in err.split("\n") if "zstd input %d on the device: window" % i in ln]
            assert len(rows) == int(want["windows"]) and all("checksum" in ln and "execution" in ln for ln in rows), err
        assert err.count("handed back at -") == len(names) and "zstd on the device: " not in err and "NOT taken" not in err, err
    return dev, err


def test_single_fastq_a_window_per_block(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"])
    assert dev.returncode == 0
    kept = kept_files(tmp_path / "device")[0].read_bytes()
    assert kept.count(b"\n") % 4 == 0 and 50 < kept.count(b"\n") // 4 < 1600  # some records, not all


def test_single_fastq_windows_of_several_blocks(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"], window=100000)
    assert dev.returncode == 0


def test_the_golden_fasta(inputs, tmp_path):
    """535 compressed bytes in one block: above --zstd-window 1, so it is streamed, in the one window a block makes"""
    dev, err = compare(inputs, tmp_path, ["sample.fasta.zst"], min_windows=1)
    assert dev.returncode == 0 and len(kept_files(tmp_path / "device")) == 1  # (the pattern is not in it: compare() has checked the empty output and the logs)


def test_pair_both_streamed_side_by_side(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst", "mate.fastq.zst"])
    assert dev.returncode == 0


def test_two_frames_with_the_seam_inside_a_record(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["frames.fastq.zst"])
    assert dev.returncode == 0 and " 2 frames closed," in err, err


def test_records_span_the_windows_seams(inputs, tmp_path):
    """a window's text is a block of 128 KiB and a record is ~330 bytes: the windows' sizes say that the seams cut records, and the
    output above is --host-codec's all the same"""
    d, _ = inputs
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"], extra=["-v"], against_plain=False)
    assert dev.returncode == 0
    text = (d / "single.fastq").read_bytes()
    sizes = [int(ln.split("taken, ")[1].split(" text bytes")[0]) for ln in err.split("\n") if "zstd input 0 on the device: window" in ln]
    assert sum(sizes) == len(text) and len(sizes) >= 4
    seams, at = 0, 0
    for s in sizes[:-1]:
        at += s
        seams += text[at - 1:at] != b"\n" or text[at:at + 1] != b"@"
    assert seams >= 3, sizes


def test_bgzf_output(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["single.fastq.zst"], extra=["-z"])
    assert dev.returncode == 0 and [f for f in kept_files(tmp_path / "device") if f.name.endswith(".gz")]


def test_a_file_below_the_window_takes_the_one_shot_row(inputs, tmp_path):
    dev, err = compare(inputs, tmp_path, ["small.fastq.zst"], window=1 << 20, streamed=False)
    assert dev.returncode == 0
    assert "zstd on the device: " in err and "window by window" not in err and "zstd input 0 on the device: window" not in err, err


def test_a_late_flipped_bit_is_libzstds_error(inputs, tmp_path):
    """the windows in front of the damage are taken, then the stream hands the file back and libzstd words the error: the same
    message and exit status as --host-codec"""
    dev, err = compare(inputs, tmp_path, ["damaged.fastq.zst"], streamed=False)
    assert dev.returncode != 0
    assert err.count("zstd input 0 on the device: window") >= 3 and "libzstd reads on" in err, err
