"""`merkurio extract -z`: the kept records written as BGZF members that end at record ends.  The reference's extract fixtures
(the ones test_cli_gpu.py runs) with -z: the output, read by Python's gzip (every member, CRC-32 and ISIZE checked by zlib), is the
golden output; it ends with the 28-byte EOF member; the device codec, the host reader (--host-ingest) and zlib on the host threads
(--host-codec, the checker) agree on the text; every member starts at a record start."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from merkurio_amd import native as mk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
MODES = [[], ["--host-ingest"], ["--host-codec"]]
MODE_IDS = ["device", "host-ingest", "host-codec"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build
    build.build_all()
    if mk.device_count() < 1:
        pytest.fail("no HIP device visible")


def run(args, check=True):
    p = subprocess.run([BIN] + args, capture_output=True)
    if check and p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    return p


def text_of(blob):
    """the inflated members; asserted: whole BGZF members only, the last one the EOF member"""
    mem, used, _ = mk.bgzf_members(blob)
    assert used == len(blob) and blob[-28:] == mk.bgzf_eof() and int(mem[-1]["isize"]) == 0
    return gzip.decompress(blob)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,extra", [("simple", []), ("simple-inv", ["-v"])])
def test_fasta_fixtures(golden, tmp_path, name, extra, mode):
    fx = os.path.join(golden, "fixtures")
    out = tmp_path / f"{name}.extracted.fasta"
    run(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-r", "-s", "ACG", *extra, "-z", *mode, "-o", str(out)])
    assert not out.exists()  # the name is what is derived today plus .gz
    assert text_of((tmp_path / f"{name}.extracted.fasta.gz").read_bytes()) == open(os.path.join(fx, f"extract/{name}.extracted.fasta"), "rb").read()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fixed_width_with_logs(golden, tmp_path, mode):
    """the logs are what they are without -z"""
    fx = os.path.join(golden, "fixtures")
    args = ["extract", "-i", os.path.join(fx, "input/fixed-width.faa"), "-s", "DKAT"]
    run(args + ["-o", str(tmp_path / "plain.faa"), "-l", str(tmp_path / "plain.log")])
    run(args + ["-z", *mode, "-o", str(tmp_path / "fw.faa"), "-l", str(tmp_path / "z.log")])
    assert text_of((tmp_path / "fw.faa.gz").read_bytes()) == open(os.path.join(fx, "extract/fixed-width.extracted.faa"), "rb").read()
    body = lambda p: open(p, "rb").read().split(b"\n", 4)[4]
    assert body(tmp_path / "z.log") == body(tmp_path / "plain.log")


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_paired_input_writes_two_gz_files(golden, tmp_path, mode):
    fx = os.path.join(golden, "fixtures")
    run(["extract", "-i", os.path.join(fx, "input/paired-1.fastq"), "-2", os.path.join(fx, "input/paired-2.fastq"), "-s", "CTT", "-z", *mode,
         "-o", str(tmp_path / "paired.extracted.fastq")])
    for k in (1, 2):
        assert text_of((tmp_path / f"paired_{k}.extracted.fastq.gz").read_bytes()) == open(os.path.join(fx, f"extract/paired_{k}.extracted.fastq"), "rb").read()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_nothing_kept_gives_the_eof_member_alone(golden, tmp_path, mode):
    fx = os.path.join(golden, "fixtures")
    run(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-s", "A", "C", "G", "T", "-v", "-z", *mode, "-o", str(tmp_path / "none.fasta")])
    assert (tmp_path / "none.fasta.gz").read_bytes() == mk.bgzf_eof()


def test_members_go_to_stdout_without_an_output_path(golden):
    fx = os.path.join(golden, "fixtures")
    p = run(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-r", "-s", "ACG", "-z"])
    assert text_of(p.stdout) == open(os.path.join(fx, "extract/simple.extracted.fasta"), "rb").read()


def test_suppress_output_is_refused(golden, tmp_path):
    fx = os.path.join(golden, "fixtures")
    p = run(["extract", "-i", os.path.join(fx, "input/simple.fasta"), "-s", "ACG", "-S", "-z", "-l", str(tmp_path / "x.log")], check=False)
    assert p.returncode == 2 and b"the argument '--suppress-output' cannot be used with '--bgzf-output'" in p.stderr


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_members_of_many_records_start_at_record_starts(tmp_path, mode):
    """6 000 FASTQ records of 331 bytes, two thirds kept: 27 members; the three modes give the same text and the same cuts"""
    rng = np.random.default_rng(11)
    recs = []
    for r in range(6000):
        seq = "".join(rng.choice(list("ACGT"), size=150)) if r % 3 else "ACGT" * 37 + "GATTACAGATTACAGG"[:2]
        name = f"@r{r:07d}".ljust(331 - 150 * 2 - 5, "x")
        recs.append(f"{name}\n{seq}\n+\n{'I' * 150}\n")
    assert all(len(x) == 331 for x in recs)
    src = tmp_path / "reads.fastq"
    src.write_text("".join(recs))
    run(["extract", "-i", str(src), "-s", "ACGTACGTACGTACGTACGT", "-v", "-z", *mode, "-o", str(tmp_path / "kept")])
    blob = (tmp_path / "kept.fastq.gz").read_bytes()
    kept = "".join(x for r, x in enumerate(recs) if r % 3).encode()
    assert text_of(blob) == kept
    mem, _, _ = mk.bgzf_members(blob)
    cuts = mk.bgzf_record_cuts(np.arange(1, 4001, dtype=np.uint64) * 331)
    assert mem["isize"][:-1].tolist() == np.diff(cuts).tolist() and len(cuts) == 28
    assert all(int(c) % 331 == 0 for c in cuts)
