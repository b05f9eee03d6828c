"""The host loop of `merkurio tag` (cli/tag_host.cpp) runs from where the reader stands to where it ends, and the reader can be given an
end (SamFile::seek_text / seek_bam): that is how a window the device refused is tagged by the host loop alone while the windows around
it stay on the device (cli/tag_windows.cpp).  Without a GPU (tests/helpers/tag_turn_harness.cpp: a matcher stub that keeps every
record): the whole file through the loop in one go and the same file as 1, 2 and 7 bounded turns one after the other give the same
output, for SAM and BAM input and SAM and BAM output; BAM turns are cut at BGZF members, so records cross the cuts and are carried
over as the next turn's head.  MERKURIO_TEST_SANITIZE=1 builds the harness with ASan + UBSan; the program is run directly."""
import gzip
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cli_sources import reader_sources
from tag_windows import EOF, NIB, _bgzf, bam_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FLAGS = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
          if os.environ.get("MERKURIO_TEST_SANITIZE") else ["-O1"])
HEADER = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000000\n"
N = 6000


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("turn")
    cli_dir = os.path.join(ROOT, "merkurio_amd/csrc/cli")
    exe = str(d / "tag_turn_harness")
    subprocess.run(["g++", "-std=c++17", *_FLAGS, "-w", "-I", cli_dir, "-o", exe, os.path.join(ROOT, "tests/helpers/tag_turn_harness.cpp"),
                    os.path.join(cli_dir, "tag_host.cpp"), *reader_sources()], check=True)
    rnd = random.Random(11)
    lines, recs = [], bytearray()
    for i in range(N):
        L = rnd.choice((100, 131, 150))
        seq = "".join(rnd.choice("ACGT") for _ in range(L))
        aux_t = ["NM:i:%d" % (i % 40), "RG:Z:g%d" % (i % 3)][:i % 3] + (["km:Z:OLD%d" % i] if i % 50 == 0 else [])
        aux_b = [b"NMC" + bytes([i % 40]), b"RGZg%d\0" % (i % 3)][:i % 3] + ([b"kmZOLD%d\0" % i] if i % 50 == 0 else [])
        lines.append("\t".join([f"r{i}", "0", "chr1", str(i + 1), "60", f"{L}M", "*", "0", "0", seq, "I" * L] + aux_t) + "\n")
        recs += bam_record(b"r%d" % i, seq.encode(), qual=bytes([40] * L), aux=b"".join(aux_b), cigar=(L << 4,), pos=i, flag=0)
    (d / "in.sam").write_text(HEADER + "".join(lines))
    ht = HEADER.encode()
    raw = b"BAM\1" + len(ht).to_bytes(4, "little") + ht + (1).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"chr1\0" + (100000000).to_bytes(4, "little")
    (d / "in.bam").write_bytes(_bgzf(raw + bytes(recs)) + EOF)
    return d, exe


def run(d, exe, inp, out, turns):
    p = subprocess.run([exe, str(d / inp), str(d / out), str(turns), "1"], capture_output=True, text=True, check=True)
    assert "#error" not in p.stdout and f"#records {N}" in p.stdout, p.stdout + p.stderr
    heads = [int(ln.split()[3]) for ln in p.stdout.split("\n") if ln.startswith("#turn")]
    assert len(heads) == turns
    data = open(d / out, "rb").read()
    return (gzip.decompress(data) if out.endswith(".bam") else data), heads


@pytest.mark.parametrize("inp", ["in.sam", "in.bam"])
@pytest.mark.parametrize("ext", ["sam", "bam"])
def test_bounded_turns_concatenate_to_the_whole_file(job, inp, ext):
    d, exe = job
    whole, _ = run(d, exe, inp, f"whole_{inp[3:]}.{ext}", 0)
    assert whole.count(b"OLD") == 2 * (N // 50) and len(whole) > N * 150  # (the old field stays, the new one repeats its value)
    for turns in (1, 2, 7):
        got, heads = run(d, exe, inp, f"t{turns}_{inp[3:]}.{ext}", turns)
        assert got == whole, (inp, ext, turns)
        if inp == "in.bam" and turns > 1:  # records cross the cuts: members of 65 280 bytes, records of 200 to 300
            assert any(h > 0 for h in heads[1:]), heads
