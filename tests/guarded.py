"""Guarded output buffers and the capacity protocol of tests/test_gpu_capacity.py.

A buffer is `alloc` elements of payload followed by a guard of at least 4 KiB, the whole filled with a fixed non-zero byte
pattern of period 7 (several outputs are zero-initialised; a period that is no power of two also shows a copy that landed
shifted).  A call is handed the pointer and a capacity of `cap <= alloc` elements; afterwards the buffer says whether the guard
is intact and whether anything at element `cap` or above was written -- inside the payload or behind it.
"""
import numpy as np

GUARD_BYTES = 4096
PATTERN = np.frombuffer(b"\xa5\x5a\xc3\x3c\x96\x69\xe1", dtype=np.uint8)


def pattern(n_bytes):
    return np.resize(PATTERN, n_bytes)


class HostBuf:
    """numpy: `alloc` elements of `dtype`, then the guard"""

    def __init__(self, dtype, alloc, guard=GUARD_BYTES):
        self.dtype = np.dtype(dtype)
        self.alloc = int(alloc)
        self.n_payload = self.alloc * self.dtype.itemsize
        self.raw = pattern(self.n_payload + guard).copy()
        self.ptr = self.raw.ctypes.data

    def bytes_now(self):
        return self.raw

    def view(self, n=None):
        n = self.alloc if n is None else int(n)
        assert n <= self.alloc
        return self.bytes_now()[:n * self.dtype.itemsize].view(self.dtype)

    def guard_intact(self):
        b = self.bytes_now()
        return bool(np.array_equal(b[self.n_payload:], pattern(len(b))[self.n_payload:]))

    def untouched_from(self, k):
        """no byte of element k or above, payload or guard, differs from the pattern"""
        b = self.bytes_now()
        a = min(int(k), self.alloc) * self.dtype.itemsize
        return bool(np.array_equal(b[a:], pattern(len(b))[a:]))

    def first_touched_from(self, k):
        b = self.bytes_now()
        a = min(int(k), self.alloc) * self.dtype.itemsize
        bad = np.nonzero(b[a:] != pattern(len(b))[a:])[0]
        return None if not len(bad) else (a + int(bad[0])) / self.dtype.itemsize


class DeviceBuf(HostBuf):
    """torch: the same on the device.  The payload starts at the allocation's first byte (the caching allocator's blocks are
    512-byte aligned: the 16 bytes mk_scan_device asks of d_hits and d_seq, the 4 of d_rec_flags); an `alloc` that is not a
    multiple of `pad_to` elements is rounded up, as d_rec_flags' allocation must be."""

    def __init__(self, torch, dtype, alloc, guard=GUARD_BYTES, pad_to=1, device="cuda:0"):
        self.dtype = np.dtype(dtype)
        self.alloc = (int(alloc) + pad_to - 1) // pad_to * pad_to
        self.n_payload = self.alloc * self.dtype.itemsize
        self.t = torch.from_numpy(pattern(self.n_payload + guard).copy()).to(device)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def bytes_now(self):
        return self.t.cpu().numpy()


# ---------------------------------------------------------------------------- the protocol for calls with host outputs
class Outcome:
    """what one call left behind: its return code, the need it states per output, its results (when it returned MK_OK) and the
    buffers it was given"""

    def __init__(self, rc, needs, results, bufs, err):
        self.rc, self.needs, self.results, self.bufs, self.err = rc, needs, results, bufs, err


class Protocol:
    """One entry point with capacities.  `outputs`: {name: [(buffer name, dtype, extra elements)]} -- the buffers that share the
    capacity `name` (rows and row_name; rec_start with its cap + 1 entries and keep).  `invoke(caps, bufs)` makes the call
    with fresh counters and returns (rc, {name: stated need}, results); bufs[buffer name] is the guarded HostBuf and invoke
    reads the results out of them itself.  `states_all`: the header promises every need after the first refusal.
    `work_done`: (names, of_R) -- the outputs whose refusal the header says leaves the call's work done: invoke then puts
    bufs["_partial"] = (keep, the rows it was given room for, counters) and of_R(R) gives the same three of a call that fit."""

    def __init__(self, mk, outputs, invoke, ample, states_all=False, work_done=((), None)):
        self.mk, self.outputs, self.invoke, self.ample, self.states_all, self.work_done = mk, outputs, invoke, ample, states_all, work_done
        self.calls = 0

    def call(self, caps, alloc=None):
        alloc = alloc or caps
        bufs = {}
        for name, members in self.outputs.items():
            for bname, dtype, extra in members:
                bufs[bname] = HostBuf(dtype, max(alloc[name], caps[name]) + extra)
        err0 = set_sentinel_error(self.mk)
        rc, needs, results = self.invoke(dict(caps), bufs)
        self.calls += 1
        err = self.mk.load().mk_last_error() if rc else b""
        assert not rc or err != err0, "the failed call left no message of its own"
        return Outcome(rc, needs, results, bufs, err)

    def check_bufs(self, o, caps, what):
        for name, members in self.outputs.items():
            for bname, _, extra in members:
                b = o.bufs[bname]
                assert b.guard_intact(), f"{what}: the guard behind {bname} was written"
                assert b.untouched_from(caps[name] + extra), \
                    f"{what}: {bname} was written at element {b.first_touched_from(caps[name] + extra)}, its capacity is {caps[name]} (+{extra})"

    def run(self, expected, oracle_needs):
        """the five steps; `expected`: the oracle's results in the form `invoke` returns them; oracle_needs: {name: N} derived from
        the oracle's result (a name may be missing where no second derivation exists).  Returns (R, N)."""
        mk = self.mk
        names = list(self.outputs)
        # 1. ample
        ample = {k: self.ample[k] for k in names}
        o = self.call(ample)
        assert o.rc == mk.MK_OK, (o.rc, o.err)
        R, N = o.results, {k: int(o.needs[k]) for k in names}
        assert R == expected, "the ample run differs from the oracle"
        for k, v in oracle_needs.items():
            assert N[k] == v, f"need of {k}: the call states {N[k]}, the oracle's result gives {v}"
        assert all(N[k] >= 2 for k in names), N
        assert all(N[k] * 4 <= ample[k] for k in names), (N, ample)
        self.check_bufs(o, ample, "ample")
        # 2. exact fit
        o = self.call(N)
        assert o.rc == mk.MK_OK, ("exact fit", N, o.rc, o.err)
        assert o.results == R, "exact fit: results differ from the ample run"
        assert {k: int(o.needs[k]) for k in names} == N
        self.check_bufs(o, N, "exact fit")
        # 3. one short, 4. the same handle afterwards
        for k in names:
            for cap in (N[k] - 1, 0, N[k] // 2):
                caps = dict(N)
                caps[k] = cap
                o = self.call(caps, alloc=N)
                what = f"{k} = {cap} of {N[k]}"
                assert o.rc == mk.MK_E_CAPACITY, (what, o.rc, o.err)
                assert int(o.needs[k]) == N[k], f"{what}: the call states a need of {o.needs[k]}"
                assert str(N[k]).encode() in o.err, f"{what}: the message does not name the need: {o.err}"
                self.check_bufs(o, caps, what)
                if k in self.work_done[0]:
                    keep_R, rows_R, counters_R = self.work_done[1](R)
                    keep, rows, counters = o.bufs["_partial"]
                    assert keep == keep_R, f"{what}: keep of the refused call"
                    assert rows == rows_R[:len(rows)] and len(rows) == min(caps.get("rows", 0), len(rows_R)), f"{what}: rows[0, rows_cap) of the refused call"
                    assert counters == counters_R, f"{what}: counters of the refused call"
                if self.states_all:
                    assert {j: int(o.needs[j]) for j in names} == N, what
                o = self.call(N)
                assert o.rc == mk.MK_OK and o.results == R, f"after the refusal at {what}: the next call differs"
                self.check_bufs(o, N, "after " + what)
        # 5. several outputs too small at once: the callers' loop -- grow what the call reports as too small, call again
        if len(names) > 1:
            for start in (0, None):
                caps = {k: (0 if start == 0 else N[k] // 2) for k in names}
                for attempt in range(len(names) + 1):
                    o = self.call(caps, alloc=N)
                    if attempt == 0 and self.states_all:
                        assert o.rc == mk.MK_E_CAPACITY and {j: int(o.needs[j]) for j in names} == N, (caps, o.needs)
                    if o.rc != mk.MK_E_CAPACITY:
                        break
                    self.check_bufs(o, caps, f"loop at {caps}")
                    grown = False
                    for k in names:
                        if int(o.needs[k]) > caps[k]:
                            assert int(o.needs[k]) == N[k], (k, o.needs[k], N[k])
                            caps[k], grown = int(o.needs[k]), True
                    assert grown, f"MK_E_CAPACITY at {caps} without a need above a capacity: {o.needs}"
                assert o.rc == mk.MK_OK, f"the loop from {start} did not end within {len(names) + 1} calls: {caps} of {N}, {o.err}"
                assert o.results == R
                self.check_bufs(o, caps, "end of the loop")
        return R, N


def rows_list(rows):
    return list(zip(rows["file"].tolist(), rows["rec"].tolist(), rows["pat"].tolist(), rows["pos"].tolist()))


def set_sentinel_error(mk):
    """mk_last_error() is a thread's last message and a call that succeeds does not clear it: a cheap call that fails on purpose
    (a NULL handle) sets a known one, so that the message read after a refusal is shown to be that refusal's"""
    lib = mk.load()
    assert lib.mk_tag_value(None, None, 0, None, None, 0, None) == mk.MK_E_INVALID_ARG
    return lib.mk_last_error()
