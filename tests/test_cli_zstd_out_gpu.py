"""`merkurio extract --zstd-output`: the kept records written as zstd frames that end at record ends, compressed on the device
(mk_zstd_deflate_records) or, with --host-codec, by libzstd level 3 at the same cuts (the checker).  FASTQ, FASTA and a pair: the
device's frames, libzstd's frames and the plain output are the same text; every frame decodes alone and ends at a record end; the .zst
fed back through --device-zstd gives the same kept records; a job that keeps nothing writes one empty frame; -z and -S exclude the flag;
the timing row of the device codec is there (a build that silently wrote with libzstd would not print it)."""
import os
import subprocess

import pytest

import zstd_cases as zc
import zstd_out_cases as zo
from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build
    build.build_all()
    if mk.device_count() < 1:
        pytest.fail("no HIP device visible")


def run(args, check=True, timing=False):
    env = dict(os.environ, MERKURIO_TIMING="1") if timing else None
    p = subprocess.run([BIN] + args, capture_output=True, env=env)
    if check and p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    return p


def text_of(blob, own_format):
    """the text of every frame, each decoded alone; own_format: the frames are this writer's (one block, descriptor 0xA4)"""
    frames = zo.frames_by_libzstd(blob)
    if own_format:
        for f, t in frames:
            assert zo.shape(f)["text"] == len(t) <= zo.TEXT_MAX - 1
    return b"".join(t for _, t in frames), frames


def three_ways(args, out, names, tmp_path):
    """plain, --zstd-output and --zstd-output --host-codec -> the plain text per output file, asserted equal three times"""
    texts = []
    for sub, extra in (("plain", []), ("dev", ["--zstd-output"]), ("host", ["--zstd-output", "--host-codec"])):
        d = tmp_path / sub
        d.mkdir()
        run(args + extra + ["-o", str(d / out)])
        if not extra:
            texts.append([(d / n).read_bytes() for n in names])
            continue
        assert not any((d / n).exists() for n in names)  # the name is the derived one plus .zst
        got = [text_of((d / (n + ".zst")).read_bytes(), sub == "dev") for n in names]
        texts.append([t for t, _ in got])
        for t, frames in got:  # every frame is whole records: it starts where a record starts
            assert all(ft[:1] in (b"@", b">") for _, ft in frames if ft)
    assert texts[0] == texts[1] == texts[2] and all(texts[0])
    return texts[0]


def test_fastq_three_ways_and_back_through_the_device_decoder(tmp_path):
    src = tmp_path / "reads.fastq"
    src.write_bytes(zc.fastq(4000))  # about 1.3 MB: the kept records take several frames
    args = ["extract", "-i", str(src), "-s", "ACGT"]
    (kept,) = three_ways(args, "hits.fastq", ["hits.fastq"], tmp_path)
    assert len(kept) > 3 * zo.GRID
    back = tmp_path / "back"
    back.mkdir()
    run(["extract", "-i", str(tmp_path / "dev" / "hits.fastq.zst"), "--device-zstd", "-s", "ACGT", "-o", str(back / "again.fastq")])
    (again,) = list(back.iterdir())  # (the name's extension is derived from the input's)
    assert again.read_bytes() == kept


def test_fasta_fixture_three_ways(golden, tmp_path):
    fx = os.path.join(golden, "fixtures")
    (kept,) = three_ways(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-r", "-s", "ACG"], "simple.extracted.fasta", ["simple.extracted.fasta"], tmp_path)
    assert kept == open(os.path.join(fx, "extract/simple.extracted.fasta"), "rb").read()


def test_pair_three_ways(golden, tmp_path):
    fx = os.path.join(golden, "fixtures")
    names = ["paired_1.extracted.fastq", "paired_2.extracted.fastq"]
    kept = three_ways(["extract", "-i", os.path.join(fx, "input/paired-1.fastq"), "-2", os.path.join(fx, "input/paired-2.fastq"), "-s", "CTT"],
                      "paired.extracted.fastq", names, tmp_path)
    for k, t in zip((1, 2), kept):
        assert t == open(os.path.join(fx, f"extract/paired_{k}.extracted.fastq"), "rb").read()


def test_without_o_the_frames_go_to_stdout(golden):
    fx = os.path.join(golden, "fixtures")
    args = ["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-r", "-s", "ACG"]
    assert text_of(run(args + ["--zstd-output"]).stdout, True)[0] == run(args).stdout != b""


@pytest.mark.parametrize("mode", [[], ["--host-codec"]], ids=["device", "host-codec"])
def test_an_empty_result_is_one_empty_frame(golden, tmp_path, mode):
    fx = os.path.join(golden, "fixtures")
    run(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-s", "ACGTTGCAACGTTGCAACGTTGCAACGTTGC", "--zstd-output", *mode, "-o", str(tmp_path / "none.fasta")])
    blob = (tmp_path / "none.fasta.zst").read_bytes()
    frames = zo.frames_by_libzstd(blob)
    assert len(blob) == 16 and [t for _, t in frames] == [b""] and zo.shape(blob)["block"] == 0
    assert zc.libzstd_says(blob) == b""


def test_exclusions(golden, tmp_path):
    fx = os.path.join(golden, "fixtures")
    base = ["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-s", "ACG", "--zstd-output"]
    p = run(base + ["-z", "-o", str(tmp_path / "x.fasta")], check=False)
    assert p.returncode != 0 and b"'--bgzf-output' cannot be used with '--zstd-output'" in p.stderr
    p = run(base + ["-S", "-l", str(tmp_path / "x.log")], check=False)
    assert p.returncode != 0 and b"'--suppress-output' cannot be used with '--zstd-output'" in p.stderr
    assert not list(tmp_path.glob("*.zst"))


def test_the_timing_row_names_the_device_codec(tmp_path):
    src = tmp_path / "reads.fastq"
    src.write_bytes(zc.fastq(1200))
    p = run(["extract", "-i", str(src), "-s", "ACGT", "--zstd-output", "-o", str(tmp_path / "t.fastq")], timing=True)
    rows = [l for l in p.stderr.decode().splitlines() if l.startswith("[timing] zstd output")]
    assert len(rows) == 1 and "(device codec)" in rows[0], p.stderr.decode()[-2000:]
    n_frames = len(zo.frames_by_libzstd((tmp_path / "t.fastq.zst").read_bytes()))
    assert n_frames >= 2 and f"{n_frames} frames written" in rows[0] and f"compressed {n_frames}," in rows[0]
    p = run(["extract", "-i", str(src), "-s", "ACGT", "--zstd-output", "--host-codec", "-o", str(tmp_path / "h.fastq")], timing=True)
    assert "[timing] zstd output (libzstd, host)" in p.stderr.decode()
