"""`merkurio tag` with plain SAM input and SAM / STDOUT / -S output keeps a window's lines on the device (mk_tag_sam_window,
cli/tag_windows.cpp: tag_sam_windows_on_device) unless --host-ingest asks for the host loop: both must give the same bytes -- output,
text log body, the stable parts of the JSON log -- and the same errors.  Under MERKURIO_TIMING=1 the window path prints a row of
its own, which is how these tests know which path ran."""
import json
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "merkurio_amd", "lib", "merkurio")
WINDOW_ROW = b"SAM text windows on the device"


@pytest.fixture(scope="module", autouse=True)
def _built():
    from merkurio_amd import build, native
    build.build_all()
    if native.device_count() < 1:
        pytest.fail("no HIP device visible")


def run(args, check=True, timing=True):
    env = dict(os.environ)
    if timing:
        env["MERKURIO_TIMING"] = "1"
    else:
        env.pop("MERKURIO_TIMING", None)
    p = subprocess.run([BIN] + args, capture_output=True, env=env)
    if check and p.returncode != 0:
        raise AssertionError(f"merkurio {' '.join(args)} -> {p.returncode}\n{p.stderr.decode()}")
    return p


def sam_without_own_pg(data):
    return [ln for ln in data.split(b"\n") if not ln.startswith(b"@PG\tID:merkurio")]


def log_body(path):
    return open(path, "rb").read().split(b"\n", 4)[4]


def json_stable(path):
    t = open(path, "rb").read()
    head, rest = t.split(b'  "meta_information": ', 1)
    key = b'  "pattern_hit_counts": '
    return head, key + rest.split(key, 1)[1]


def make_lines(rnd, kmers, n):
    """the 40 000 lines of test_cli_gpu.py::test_tag_is_batched"""
    lines = []
    for i in range(n):
        s = "".join(rnd.choice("ACGTacgt" if i % 50 == 0 else "ACGT") for _ in range(rnd.choice((50, 150))))
        if i % 4 == 0:
            k = rnd.choice(kmers)
            o = rnd.randrange(len(s) - 31)
            s = s[:o] + k + s[o + 31:]
        extra = "\tkm:Z:OLD" if i % 1000 == 0 else ""
        lines.append(f"r{i}\t4\t*\t0\t0\t*\t*\t0\t0\t{s}\t{'I' * len(s)}{extra}\n")
    return lines


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    d = tmp_path_factory.mktemp("samwin")
    rnd = random.Random(5)
    kmers = ["".join(rnd.choice("ACGT") for _ in range(31)) for _ in range(200)]
    lines = make_lines(rnd, kmers, 40000)
    (d / "in.sam").write_text("@HD\tVN:1.6\n@SQ\tSN:1\tLN:100000\n" + "".join(lines))
    (d / "k.txt").write_text("\n".join(kmers) + "\n")
    return d, lines


def both(d, tag, extra, stdout=False, suppress=False):
    """the same command on the window path and with --host-ingest -> [(output, log body, stable JSON, stderr)] * 2"""
    res = []
    for mode, flags in (("dev", []), ("host", ["--host-ingest"])):
        o = d / f"{tag}_{mode}.sam"
        lg, js = d / f"{tag}_{mode}.log", d / f"{tag}_{mode}.json"
        args = ["tag", "-i", str(d / "in.sam"), "-f", str(d / "k.txt"), "-l", str(lg), "-j", str(js), *extra, *flags]
        if suppress:
            args += ["-S"]
        elif not stdout:
            args += ["-o", str(o)]
        p = run(args)
        data = p.stdout if stdout else (b"" if suppress else o.read_bytes())
        res.append((sam_without_own_pg(data), log_body(lg), json_stable(js), p.stderr))
    return res


@pytest.mark.parametrize("extra", [[], ["-m"], ["-v"], ["--gpus", "2"], ["--window-mb", "1"], ["--window-mb", "1", "-m"],
                                   ["--window-mb", "1", "--gpus", "2", "-v"]], ids=lambda e: "_".join(e).replace("-", "") or "default")
def test_window_path_equals_host_path(job, extra):
    d, lines = job
    tag = "o" + "".join(extra).replace("-", "")
    dev, host = both(d, tag, extra)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    if "--window-mb" in extra:  # (11 MB of text: many windows)
        row = [ln for ln in dev[3].split(b"\n") if WINDOW_ROW in ln][0].split()
        assert row[1] == row[3] and int(row[1]) > 5, row
    assert b"left to the host reader" not in dev[3]
    assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2]
    recs = [ln for ln in dev[0] if ln and not ln.startswith(b"@")]
    if "-m" in extra:
        assert 9000 < len(recs) < 40000 and all(b"\tkm:Z:" in ln for ln in recs)
    elif "-v" in extra:
        assert 20000 < len(recs) < 40000 and all(ln.endswith(b"\tkm:Z:") or ln.endswith(b"\tkm:Z:OLD") for ln in recs)
    else:
        assert len(recs) == 40000 and any(b",OLD" in ln or b"km:Z:OLD," in ln for ln in recs)


def test_stdout_and_suppressed_output(job):
    d, _ = job
    dev, host = both(d, "so", ["--window-mb", "2"], stdout=True)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    assert dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2] and len(dev[0]) > 40000
    dev, host = both(d, "sup", ["--window-mb", "2"], suppress=True)
    assert WINDOW_ROW in dev[3] and WINDOW_ROW not in host[3]
    assert dev[0] == host[0] == [b""] and dev[1] == host[1] and dev[2] == host[2]
    stats = json.loads(open(d / "sup_dev.json", "rb").read())
    assert stats  # (a complete JSON document)


def test_refused_windows_fall_back_to_the_host_loop(job, tmp_path):
    """a 9-field line in window 3: the window path hands the input to the host loop there, which ends the job with the host path's
    error; `km:i:5` on a record that -v drops is not looked at by either path"""
    d, lines = job
    rnd = random.Random(7)
    size, k = 0, 0
    while size < 3 * (1 << 20) + 1000:  # the first line that lies in the fourth 1 MiB window
        size += len(lines[k])
        k += 1
    bad = list(lines)
    bad[k] = "\t".join(bad[k].rstrip("\n").split("\t")[:9]) + "\n"
    (tmp_path / "bad.sam").write_text("@HD\tVN:1.6\n" + "".join(bad))
    res = []
    for flags in ([], ["--host-ingest"]):
        p = run(["tag", "-i", str(tmp_path / "bad.sam"), "-f", str(d / "k.txt"), "-o", str(tmp_path / "bad_out.sam"), "--window-mb", "1", *flags], check=False)
        res.append(p)
    assert res[0].returncode == res[1].returncode != 0
    msg = [[ln for ln in p.stderr.split(b"\n") if ln and not ln.startswith(b"[timing]")] for p in res]
    assert msg[0] == msg[1] and any(b"too few fields" in ln for ln in msg[0])
    assert b"left to the host reader (a line with too few fields)" in res[0].stderr and WINDOW_ROW in res[0].stderr
    # km:i:5 on a record with a hit, under -v (dropped): the same bytes; without -v it is kept and both paths refuse it alike
    hit = next(i for i in range(k, len(lines)) if i % 4 == 0 and i % 1000 != 0)
    odd = list(lines)
    odd[hit] = odd[hit].rstrip("\n") + "\tkm:i:5\n"
    (tmp_path / "odd.sam").write_text("@HD\tVN:1.6\n" + "".join(odd))
    outs = []
    for mode, flags in (("dev", []), ("host", ["--host-ingest"])):
        o = tmp_path / f"odd_{mode}.sam"
        p = run(["tag", "-i", str(tmp_path / "odd.sam"), "-f", str(d / "k.txt"), "-o", str(o), "--window-mb", "1", "-v", *flags])
        outs.append(sam_without_own_pg(o.read_bytes()))
        assert (WINDOW_ROW in p.stderr) == (mode == "dev") and b"left to the host reader" not in p.stderr
    assert outs[0] == outs[1] and len(outs[0]) > 20000
    res = [run(["tag", "-i", str(tmp_path / "odd.sam"), "-f", str(d / "k.txt"), "-o", str(tmp_path / "odd_kept.sam"), "--window-mb", "1", *flags], check=False)
           for flags in ([], ["--host-ingest"])]
    assert res[0].returncode == res[1].returncode != 0
    msg = [[ln for ln in p.stderr.split(b"\n") if ln and not ln.startswith(b"[timing]")] for p in res]
    assert msg[0] == msg[1] and any(b"Invalid tag value format" in ln for ln in msg[0])
    assert b"left to the host reader (existing tag)" in res[0].stderr
