"""`merkurio tag`: a window the device refuses is tagged by the host loop ALONE, in that window's place of the output order, and the
windows behind it stay on the device (cli/tag_windows.cpp: the host turn; cli/tag_host.cpp: the loop).  All four directions, 1 MiB
windows, inputs of 6 to 8 windows: the output is --host-ingest's byte for byte (BAM: the inflated stream, the writer's own @PG line
aside), the logs are equal, and the window row under MERKURIO_TIMING=1 counts `windows: D on the device, H on the host`.  After
R = 4 refused windows in a row the rest of the file goes to the host loop as one piece.

A BAM window refused BEFORE its tail is known (a record chain the device cannot prove, a damaged member) and read by the host all
the same could not be built: every construction of tests/test_gpu_bam_window.py::test_refusals for status bits 1 and 8 is a
"truncated file" to the host parser too, and a member with a wrong stored CRC-32 is "Error while decompressing" to zlib's path.  That
case is covered by the error test below (the refusal, the host's wording, what was written before) and, for the head the host turn
hands on, by tests/test_tag_window_turn_cpu.py."""
import os
import random
import re
import struct
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cli_bam_sam_window_gpu as B
import test_cli_sam_bam_window_gpu as S

pytestmark = pytest.mark.gpu

W = 1 << 20
MEMBER = 0xff00
FIRST_MEMBER, MEMBERS_PER_WINDOW = 2, 17  # (SamFile::open inflates two members for the header; 17 members are the first run of >= 1 MiB)
R = 4
DIRECTIONS = ["bam_sam", "bam_bam", "sam_bam", "sam_sam"]
TITLES = {"bam_sam": b" BAM -> SAM text", "bam_bam": b"", "sam_bam": b" SAM text -> BAM", "sam_sam": b" SAM text"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("turn")
    rnd = random.Random(6)  # (a layout in which no window starts at a record start, with or without the longer records in front)
    kmers = [bytes(rnd.choice(b"ACGT") for _ in range(31)) for _ in range(80)]
    (d / "k.txt").write_bytes(b"\n".join(kmers) + b"\n")
    recs = B.make_records(rnd, kmers, 30000)
    lines = S.make_lines(rnd, [k.decode() for k in kmers], 21000)
    return d, recs, lines


# ---- where the windows are ------------------------------------------------------------------------------------------------------
def bam_text_head():
    text = b"BAM\1" + struct.pack("<i", len(B.HEADER)) + B.HEADER + struct.pack("<i", len(B.REFS))
    for nm, ln in B.REFS:
        text += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    return len(text)


def bam_windows(recs):
    """-> (window of every record: the one its last byte lies in, number of windows, text offsets where the windows start)"""
    at, win = bam_text_head(), []
    for r in recs:
        at += len(r)
        win.append(max(0, ((at - 1) // MEMBER - FIRST_MEMBER) // MEMBERS_PER_WINDOW))
    n_members = (at + MEMBER - 1) // MEMBER
    n = (n_members - FIRST_MEMBER + MEMBERS_PER_WINDOW - 1) // MEMBERS_PER_WINDOW
    return win, n, [(FIRST_MEMBER + MEMBERS_PER_WINDOW * k) * MEMBER for k in range(n)]


def sam_windows(lines):
    """LineInput::cut: a window ends at the first line start at or behind its start + 1 MiB -> (window of every line, number of windows)"""
    win, k, start, at = [], 0, len(S.HEADER), len(S.HEADER)
    for ln in lines:
        if at >= start + W:
            k, start = k + 1, at
        win.append(k)
        at += len(ln)
    return win, k + 1


def odd_bam(direction, recs, k):
    """record k as one the device refuses and the host takes: to SAM text a float "%g" writes as 1e-05; BAM -> BAM passes the optional
    fields through as they are and never looks at a float, so there the refusal every direction has: an existing km value above
    2 048 bytes (bam.hip: bit 4)"""
    more = b"XEf" + struct.pack("<f", 1e-5) if direction == "bam_sam" else b"kmZ" + b"A" * 2049 + b"\0"
    return struct.pack("<i", struct.unpack_from("<i", recs[k], 0)[0] + len(more)) + recs[k][4:] + more


def make_input(d, direction, recs, lines, windows, name, malformed=None):
    """the input with a refusing KEPT record (one with a planted k-mer and no km field yet) in the middle of each of `windows`
    (malformed: a window that gets a record the host loop bails on instead) -> (path, number of windows)"""
    if direction.startswith("bam"):
        odd = list(recs)
        win, n, _ = bam_windows(odd)
        for wdw in list(windows) + ([malformed] if malformed is not None else []):
            idx = [i for i, x in enumerate(win) if x == wdw]
            i = next(i for i in idx[len(idx) // 2:] if i % 4 == 0 and i % 1000)
            if wdw == malformed:
                odd[i] = struct.pack("<i", struct.unpack_from("<i", recs[i], 0)[0] + 7) + recs[i][4:] + b"kmi" + struct.pack("<i", 7)
            else:
                odd[i] = odd_bam(direction, recs, i)
        win, n, starts = bam_windows(odd)  # (a longer record moves the ones behind it: check)
        changed = sorted(win[i] for i in range(len(recs)) if odd[i] is not recs[i])
        assert changed == sorted(list(windows) + ([malformed] if malformed is not None else [])), changed
        # every window starts inside a record: the record a window's host turn stops in front of ends in the next window's first member
        at, bounds = bam_text_head(), set()
        for r in odd:
            bounds.add(at)
            at += len(r)
        assert not bounds & set(starts[1:])
        path = d / (name + ".bam")
        B.write_bam(path, odd)
        return path, n
    field = "\tXF:f:1e-45" if direction == "sam_bam" else "\tkm:Z:" + "A" * 2049  # (sam.hip: an existing value above 2 048 bytes sets bit 4)
    odd = list(lines)
    win, n = sam_windows(odd)
    for wdw in list(windows) + ([malformed] if malformed is not None else []):
        idx = [i for i, x in enumerate(win) if x == wdw]
        i = next(i for i in idx[len(idx) // 2:] if i % 4 == 0 and i % 1000)
        odd[i] = "\t".join(odd[i].rstrip("\n").split("\t")[:9]) + "\n" if wdw == malformed else odd[i].rstrip("\n") + field + "\n"
    win2, n2 = sam_windows(odd)
    assert n2 == n and all(win2[i] == win[i] for i in range(len(odd)) if odd[i] is not lines[i])
    path = d / (name + ".sam")
    path.write_text(S.HEADER + "".join(odd))
    return path, n


def tag(d, direction, inp, name, extra, flags, check=True):
    """-> (returncode, output: SAM lines | BAM parts, stable JSON or None, stderr)"""
    out = d / (name + (".bam" if direction.endswith("bam") else ".sam"))
    args = ["tag", "-i", str(inp), "-f", str(d / "k.txt"), "-o", str(out), "--window-mb", "1"]
    js = None
    for e in extra:
        if e == "-j":
            js = d / (name + ".json")
            args += ["-j", str(js)]
        else:
            args.append(e)
    p = B.run(args + flags, check=check)
    if p.returncode != 0:
        return p.returncode, out.read_bytes() if out.exists() else b"", None, p.stderr
    data = S.bam_parts(out) if direction.endswith("bam") else B.sam_without_own_pg(out.read_bytes())
    return 0, data, B.json_stable(js) if js else None, p.stderr


def counts(direction, stderr):
    """the window row -> (windows on the device, windows on the host, windows)"""
    row = re.search(rb"\[timing\] \d+ of (\d+)" + re.escape(TITLES[direction]) + rb" windows on the device \(.*", stderr)
    assert row, stderr.decode()
    m = re.search(rb"windows: (\d+) on the device, (\d+) on the host", row.group(0))
    assert m, row.group(0)  # (before there was a host turn the row had no such counts)
    return int(m.group(1)), int(m.group(2)), int(row.group(1))


def same_as_host(d, direction, inp, name, extra, dev_flags=()):
    dev = tag(d, direction, inp, name + "_dev", extra, list(dev_flags))
    host = tag(d, direction, inp, name + "_host", extra, ["--host-ingest"])
    assert dev[1] == host[1], (direction, name)
    assert dev[2] == host[2]
    assert b"windows on the device" not in host[3]
    return counts(direction, dev[3]), dev


@pytest.mark.parametrize("extra", [[], ["-m"], ["-m", "-j"]], ids=["all", "m", "m_j"])
@pytest.mark.parametrize("direction", DIRECTIONS)
def test_a_refused_window_is_the_only_one_on_the_host(job, direction, extra):
    """a refusing record in window 2, then in windows 1 and 4; in the BAM inputs the last record of every window ends in the next
    window's first member (make_input checks it): the record the host turn stops in front of"""
    d, recs, lines = job
    tagn = direction + "".join(extra).replace("-", "")
    inp, n = make_input(d, direction, recs, lines, [2], tagn + "_one")
    assert 6 <= n <= 8
    (dev_n, host_n, total), dev = same_as_host(d, direction, inp, tagn + "_one", extra)
    assert (dev_n, host_n, total) == (n - 1, 1, n)
    assert b"[timing] window 2 left to the host " in dev[3]
    inp, n = make_input(d, direction, recs, lines, [1, 4], tagn + "_two")
    (dev_n, host_n, total), dev = same_as_host(d, direction, inp, tagn + "_two", extra)
    assert (dev_n, host_n, total) == (n - 2, 2, n)
    assert b"[timing] window 1 left to the host " in dev[3] and b"[timing] window 4 left to the host " in dev[3]


@pytest.mark.parametrize("direction", ["bam_sam", "bam_bam"])
def test_the_record_that_crosses_into_the_next_window_is_the_refusing_one(job, direction):
    """the record that starts in window 2 and ends in window 3's first member is the one the device refuses -- it is window
    3's (its head), so window 3 is the host's and window 2 stands"""
    d, recs, lines = job
    win, n, _ = bam_windows(recs)
    i = next(i for i in range(len(recs)) if win[i] == 3)  # the first record that ends in window 3: it starts in window 2
    at = bam_text_head() + sum(len(r) for r in recs[:i])
    assert (at // MEMBER - FIRST_MEMBER) // MEMBERS_PER_WINDOW == 2
    odd = list(recs)
    odd[i] = odd_bam(direction, recs, i)
    win, n, _ = bam_windows(odd)
    assert win[i] == 3
    B.write_bam(d / f"cross_{direction}.bam", odd)
    (dev_n, host_n, total), dev = same_as_host(d, direction, d / f"cross_{direction}.bam", "cross_" + direction, [])
    assert (dev_n, host_n, total) == (n - 1, 1, n) and b"[timing] window 3 left to the host " in dev[3]


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_the_cap_on_refused_windows_in_a_row(job, direction):
    """R - 1 refused windows in a row and the windows behind them are the device's again; R in a row and the host loop keeps
    the file from the R-th on"""
    d, recs, lines = job
    inp, n = make_input(d, direction, recs, lines, list(range(1, R)), direction + "_below")
    assert n >= R + 2
    (dev_n, host_n, total), dev = same_as_host(d, direction, inp, direction + "_below", ["-m"])
    assert (dev_n, host_n, total) == (n - (R - 1), R - 1, n) and b"with every window behind it" not in dev[3]
    inp, n = make_input(d, direction, recs, lines, list(range(1, R + 1)), direction + "_at")
    (dev_n, host_n, total), dev = same_as_host(d, direction, inp, direction + "_at", ["-m"])
    assert (dev_n, host_n, total) == (1, n - 1, n)
    assert b"[timing] window %d left to the host " % R in dev[3] and b"with every window behind it" in dev[3]


def inflate_what_is_there(data):
    """the text of the whole BGZF members at the start of `data`"""
    out, at = b"", 0
    while at + 18 <= len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        if at + size > len(data):
            break
        out += zlib.decompress(data[at + 18:at + size - 8], -15)
        at += size
    return out


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_a_malformed_record_ends_the_job_with_the_host_error(job, direction):
    """a line of 9 fields (SAM) / a kept record whose km field is an integer (BAM) in window 3, behind a refused window 1:
    exit status and stderr are --host-ingest's, and so is what was written -- for SAM input the same bytes (the host loop's 1 MiB
    windows are cut by the rule of the device's windows); for BAM input the host loop's windows are 1 MiB of text and the device's
    17 members, so either output is the start of the other, and neither reaches the malformed record."""
    d, recs, lines = job
    inp, n = make_input(d, direction, recs, lines, [1], direction + "_bad", malformed=3)
    dev = tag(d, direction, inp, direction + "_bad_dev", [], [], check=False)
    host = tag(d, direction, inp, direction + "_bad_host", [], ["--host-ingest"], check=False)
    assert dev[0] == host[0] != 0
    msg = [[ln for ln in r[3].split(b"\n") if ln and not ln.startswith(b"[timing]")] for r in (dev, host)]
    assert msg[0] == msg[1] and any((b"too few fields" if direction.startswith("sam") else b"Invalid tag value format") in ln for ln in msg[0])
    assert b"[timing] window 1 left to the host " in dev[3] and b"[timing] window 3 left to the host " in dev[3]
    outs = []
    for r in (dev, host):
        if direction.endswith("bam"):
            text = inflate_what_is_there(r[1])
            l_text = struct.unpack_from("<i", text, 4)[0] if len(text) >= 8 else 0
            outs.append(text[8 + l_text:])
        else:
            outs.append(b"\n".join(B.sam_without_own_pg(r[1])))
    if direction.startswith("sam"):
        assert outs[0] == outs[1]
    else:
        assert outs[0].startswith(outs[1]) or outs[1].startswith(outs[0])
    # windows 0, 1 -- the host's turn -- and 2 were written, three windows of at least 1 MiB of text each (the host loop alone: what
    # lies in front of its own 1 MiB window with the record, which begins behind 3 MiB): a kept record or line is no shorter in the
    # output than in the input, except a SAM line as a BAM record, which keeps more than half (QUAL as it is, SEQ halved)
    assert min(len(outs[0]), len(outs[1])) > (3 * W // 2 if direction == "sam_bam" else 2 * W)


def test_a_damaged_member_is_refused_and_gets_the_host_error(job):
    """a member of window 3 whose stored CRC-32 is wrong -- refused by the device before any tail is known,
    the host turn's zlib words the error as --host-ingest does"""
    d, recs, lines = job
    B.write_bam(d / "crc.bam", recs)
    data = bytearray((d / "crc.bam").read_bytes())
    at, m = 0, 0
    while m < FIRST_MEMBER + 3 * MEMBERS_PER_WINDOW + 5:
        at += struct.unpack_from("<H", data, at + 16)[0] + 1
        m += 1
    size = struct.unpack_from("<H", data, at + 16)[0] + 1
    data[at + size - 8] ^= 0x01  # (the first byte of this member's CRC-32)
    (d / "crc.bam").write_bytes(bytes(data))
    dev = tag(d, "bam_sam", d / "crc.bam", "crc_dev", [], [], check=False)
    host = tag(d, "bam_sam", d / "crc.bam", "crc_host", [], ["--host-ingest"], check=False)
    assert dev[0] == host[0] != 0
    msg = [[ln for ln in r[3].split(b"\n") if ln and not ln.startswith(b"[timing]")] for r in (dev, host)]
    assert msg[0] == msg[1] and any(b"Error while decompressing" in ln for ln in msg[0])
    assert b"[timing] window 3 left to the host loop (a damaged member)" in dev[3]
    a, b = (b"\n".join(B.sam_without_own_pg(r[1])) for r in (dev, host))
    assert (a.startswith(b) or b.startswith(a)) and len(a) > 2 * W


@pytest.mark.parametrize("direction", DIRECTIONS)
def test_two_handles_per_window_turn(job, direction):
    """--gpus 2 (on a one-GPU box both handles' devices are the same card): the same bytes, the same counts"""
    d, recs, lines = job
    inp, n = make_input(d, direction, recs, lines, [2], direction + "_g2")
    (dev_n, host_n, total), dev = same_as_host(d, direction, inp, direction + "_g2", [], dev_flags=["--gpus", "2"])
    assert (dev_n, host_n, total) == (n - 1, 1, n)
