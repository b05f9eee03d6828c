"""`merkurio extract` on .bz2 inputs whose blocks are decoded on the device (mk_bzip2_inflate_device; the windows are
ranges of the text there) against `--host-codec` (libbz2 inflates the file at load): the kept records, the text log and the JSON log
byte for byte.  The [timing] row must name the device path with the number of blocks that the host harness counts: without that row
these tests would pass on a build that never leaves libbz2.  A damaged file is handed back to libbz2, which words the error; so is a
file that libbz2 takes and the device documents that it does not (a block magic inside a block's data), and the run ends as it does
under --host-codec."""
import bz2
import os
import subprocess

import pytest

import bzip2_cases as cases
import bzip2_craft as craft
from test_cli_gpu import BIN, json_stable, log_body

pytestmark = pytest.mark.gpu

PATTERN = "ACGTAC"  # (one read in ~14 of 150 bases holds it or its reverse complement)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


def fasta(n, seed):
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        seq = "".join(rng.choices("ACGT", k=rng.randrange(60, 900)))
        out.append(">contig%d len=%d\n%s\n" % (i, len(seq), "\n".join(seq[p:p + 70] for p in range(0, len(seq), 70))))
    return "".join(out).encode()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> blocks; the files lie in the returned directory.  0.3 - 0.85 MB of text each: up to nine blocks at level 1, blocks that
    start at any bit of a byte, streams of different levels behind each other"""
    d = tmp_path_factory.mktemp("bzcli")
    fq, mate = cases.fastq(2500, seed=11), cases.fastq(2500, seed=12)
    third = len(fq) // 3
    cut1, cut2 = fq.index(b"\n@read", third) + 1, fq.index(b"\n@read", 2 * third) + 1
    files = {
        "single.fastq.bz2": bz2.compress(fq, 1),
        "mate.fastq.bz2": bz2.compress(mate, 2),
        "contigs.fasta.bz2": bz2.compress(fasta(900, 5), 9),
        # (streams may end anywhere in the text: the second cut is in the middle of a record)
        "streams.fastq.bz2": bz2.compress(fq[:cut1], 1) + bz2.compress(fq[cut1:cut2 + 40], 9) + bz2.compress(fq[cut2 + 40:], 3),
    }
    damaged = bytearray(files["single.fastq.bz2"])
    damaged[len(damaged) // 2] ^= 0x10  # one bit of some block's symbols
    assert cases.libbz2_says(bytes(damaged)) is None
    count = cases.block_counter(d)
    blocks = {name: count(blob) for name, blob in files.items()}
    assert blocks["single.fastq.bz2"] >= 8 and blocks["streams.fastq.bz2"] >= 5, blocks
    files["damaged.fastq.bz2"] = bytes(damaged)
    for name, blob in files.items():
        (d / name).write_bytes(blob)
    return d, blocks


def compare(inputs, tmp_path, names, extra=(), device_takes=True):
    d, blocks = inputs
    run_dir = tmp_path / "runs"
    run_dir.mkdir()

    def go(tag, codec):
        o = run_dir / tag
        o.mkdir()
        ext = "fasta" if "fasta" in names[0] else "fastq"
        args = [BIN, "extract", "-i", str(d / names[0])] + (["-2", str(d / names[1])] if len(names) > 1 else [])
        args += ["-s", PATTERN, "-r", "-o", str(o / f"out.{ext}"), "-l", str(o / "x.log"), "-j", str(o / "x.json"), *extra, *codec]
        return subprocess.run(args, capture_output=True, env=dict(os.environ, MERKURIO_TIMING="1")), o
    dev, d_dir = go("device", [])
    host, h_dir = go("host", ["--host-codec"])
    err = dev.stderr.decode(errors="replace")
    print(err)
    assert dev.returncode == host.returncode, err
    plain = lambda e: [ln for ln in e.decode(errors="replace").split("\n") if not ln.startswith("[timing]")]
    assert plain(dev.stderr) == plain(host.stderr)
    assert "bzip2 on the device" not in host.stderr.decode(errors="replace")
    if dev.returncode != 0:
        # libbz2 meets the damage at load under --host-codec and, behind the device's refusal, after the outputs have been opened: no
        # record has been written either way
        assert all((d_dir / f).stat().st_size == 0 for f in os.listdir(d_dir) if f.startswith("out")), os.listdir(d_dir)
        return dev, err, d_dir
    assert sorted(os.listdir(d_dir)) == sorted(os.listdir(h_dir))
    for f in sorted(os.listdir(d_dir)):
        a, b = (d_dir / f).read_bytes(), (h_dir / f).read_bytes()
        if f == "x.log":
            assert log_body(d_dir / f) == log_body(h_dir / f)
        elif f == "x.json":
            assert json_stable(d_dir / f)[:2] == json_stable(h_dir / f)[:2]
        else:
            assert a == b, f
    if not device_takes:
        assert "NOT taken by the device" in err and "bzip2 on the device: " not in err, err
        return dev, err, d_dir
    rows = [ln for ln in err.split("\n") if "bzip2 on the device: " in ln]
    assert [ln.split("bzip2 on the device: ")[1].split(" blocks,")[0] for ln in rows] == [str(blocks[n]) for n in names], err
    assert all("block decode" in ln and "CRC" in ln for ln in rows), err
    return dev, err, d_dir


def test_fastq(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2"])
    assert dev.returncode == 0
    kept = (o / "out.fastq").read_bytes()
    assert kept.count(b"\n") % 4 == 0 and 100 < kept.count(b"\n") // 4 < 2500  # some records, not all


def test_fasta(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["contigs.fasta.bz2"])
    assert dev.returncode == 0 and (o / "out.fasta").stat().st_size > 0


def test_pair(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2", "mate.fastq.bz2"])
    assert dev.returncode == 0 and err.count("bzip2 on the device: ") == 2


def test_three_streams(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["streams.fastq.bz2"])
    assert dev.returncode == 0
    # the same text as the one-stream file: the same records are kept
    (tmp_path / "one").mkdir()
    one = compare(inputs, tmp_path / "one", ["single.fastq.bz2"])[2]
    assert sorted(os.listdir(o)) == sorted(os.listdir(one))
    for f in sorted(os.listdir(o)):
        if f.startswith("out"):
            assert (o / f).read_bytes() == (one / f).read_bytes(), f


def test_inverted_with_logs(inputs, tmp_path):
    dev, err, o = compare(inputs, tmp_path, ["single.fastq.bz2"], ["-v"])
    assert dev.returncode == 0


def test_a_flipped_data_bit_is_libbz2s_error(inputs, tmp_path):
    """the same message and exit status as --host-codec; the device hands the file back and says so"""
    dev, err, o = compare(inputs, tmp_path, ["damaged.fastq.bz2"])
    assert dev.returncode != 0 and "Error while decompressing" in err
    assert "NOT taken by the device" in err and "bzip2 on the device: " not in err


def test_a_block_magic_in_a_blocks_data_is_libbz2s_file_end_to_end(inputs, tmp_path):
    """a file libbz2 takes and the device hands back: a libbz2 stream that ends inside the last record's quality line, a hand-made
    stream whose symbols spell the block magic (its 14 bytes of text are quality values), and a libbz2 stream with the line's end"""
    d, _ = inputs
    name = "host-block-magic-in-the-symbols-nibble-aligned"
    crafted, tail = craft.CASES[name][0], craft.text_of(name)
    assert len(tail) == 14 and len(craft.find_magics(crafted)) == 3 and set(tail) <= set(range(65, 79))
    head = cases.fastq(400, seed=13) + b"@last lane=1\n" + b"ACGTAC" * 25 + b"\n+\n" + b"F" * 136
    blob = bz2.compress(head, 1) + crafted + bz2.compress(b"\n", 9)
    text = head + tail + b"\n"
    assert cases.libbz2_says(blob) == craft.libbz2_says(blob) == text and text.count(b"\n") == 4 * 401
    (d / "magic.fastq.bz2").write_bytes(blob)
    dev, err, o = compare(inputs, tmp_path, ["magic.fastq.bz2"], device_takes=False)
    assert dev.returncode == 0
    kept = (o / "out.fastq").read_bytes()
    assert kept.endswith(b"F" * 136 + tail + b"\n") and 10 < kept.count(b"\n") // 4 < 401  # the last record holds the pattern
