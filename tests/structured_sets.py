"""Pattern sets with the structure of real k-mer lists, and the batches that go with them (generators and checks, no tests).

Significant k-mers of an association study are the consecutive windows of a few hundred loci: pattern i at offset o + 1 and
pattern i + 1 at offset o are the same q-gram, so a key of the exact table (filter.hpp: 4-entry buckets, an overflow flag on
entry 0) carries up to `stride` entries and its home bucket overflows whatever the hash does.  A uniformly random set never
does that: every sampled q-gram is a key of its own.  The generators below are seeded and return (raw_patterns, records);
keys_per_entry() restates the key of an entry so that a test can assert that its set stresses the table at the geometry the
matcher reports, instead of passing vacuously.
"""
import collections
import random

BUCKET_ENTRIES = 4  # filter.hpp: kBucketEntries
DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"


# ---------------------------------------------------------------------------- the key of a table entry
def code2(c):
    """filter.hpp: the 2-bit code of a byte (N and G share one, so do U/T, R/C, Y/A and upper / lower case)"""
    return (c >> 1) & 3


def pack_qgram(p, o, q):
    """filter.hpp / build_tables.hip: the packed key of the q bases of p from offset o on, base i at bits 2i"""
    k = 0
    for i in range(q):
        k |= code2(p[o + i]) << (2 * i)
    return k


def pattern_keys(p, q, S):
    """the keys of the S table entries of one pattern (offsets 0..S-1)"""
    return [pack_qgram(p, o, q) for o in range(S)]


def entries_per_key(patterns, q, S):
    """key -> number of table entries (pattern, offset) that carry it"""
    per_key = collections.Counter()
    for p in patterns:
        per_key.update(pattern_keys(p, q, S))
    return per_key


def keys_per_entry(patterns, q, S):
    """histogram {entries on one key: number of distinct keys with that many}.  It needs no hash: more than BUCKET_ENTRIES
    entries on a key overflow that key's home bucket wherever the hash puts it."""
    return collections.Counter(entries_per_key(patterns, q, S).values())


def overflowing_share(patterns, q, S):
    """share of the distinct keys that carry more entries than a bucket holds"""
    h = keys_per_entry(patterns, q, S)
    return sum(n for e, n in h.items() if e > BUCKET_ENTRIES) / max(1, sum(h.values()))


def max_entries_on_a_key(patterns, q, S):
    return max(keys_per_entry(patterns, q, S))


# ---------------------------------------------------------------------------- generators
def _seq(rnd, n, alpha=DNA):
    return bytes(rnd.choice(alpha) for _ in range(n))


def _other(rnd, c, alpha):
    return rnd.choice([x for x in alpha if x != c])


def _substituted(rnd, s, alpha):
    k = rnd.randrange(len(s))
    return s[:k] + bytes([_other(rnd, s[k], alpha)]) + s[k + 1:]


def tiled(n_loci, width, k, seed=1, n_reads=300, read_len=150, alpha=DNA, flank=60, long_bytes=140_000):
    """`width` consecutive k-mers of each of n_loci random loci.  Records: read_len-base windows of the loci (with `flank`
    bases of random sequence either side) at random offsets, the same windows with one substituted base, random reads, and
    one long record of all loci with random spacers (long_bytes or more: several 31 KiB tiles, many 1 KiB chunks)."""
    rnd = random.Random(seed)
    loci = [_seq(rnd, flank + width + k - 1 + flank, alpha) for _ in range(n_loci)]
    raw = [g[flank + i:flank + i + k] for g in loci for i in range(width)]
    recs = []
    for _ in range(n_reads):
        g = rnd.choice(loci)
        n = min(read_len, len(g))
        a = rnd.randrange(0, len(g) - n + 1)
        w = g[a:a + n]
        recs.append(w)
        recs.append(_substituted(rnd, w, alpha))
        recs.append(_seq(rnd, read_len, alpha))
    gap = 2 * max(1, (long_bytes - sum(map(len, loci))) // max(1, n_loci)) if long_bytes else 0
    long_rec = bytearray()
    for g in loci:
        long_rec += _seq(rnd, rnd.randrange(0, gap + 1), alpha) + g
    while long_bytes and len(long_rec) < long_bytes:
        long_rec += _seq(rnd, 1000, alpha)
    if long_bytes:
        recs.append(bytes(long_rec))
    return raw, recs


def shared_prefix(n, prefix_len=(31, 20), total_len=60, seed=2, n_planted=160, alpha=DNA):
    """one group of n patterns per entry of prefix_len: the bare prefix and n - 1 patterns of total_len bases that begin
    with it.  Records hold the bare prefix, whole patterns, and whole patterns with their last byte changed; n_planted
    occurrences of a prefix in the whole batch at most."""
    rnd = random.Random(seed)
    lens = (prefix_len,) if isinstance(prefix_len, int) else tuple(prefix_len)
    raw, groups = [], []
    for pl in lens:
        pre = _seq(rnd, pl, alpha)
        grp = {pre}
        while len(grp) < n:
            grp.add(pre + _seq(rnd, total_len - pl, alpha))
        grp = sorted(grp)
        rnd.shuffle(grp)
        groups.append((pre, grp))
        raw += grp
    recs = []
    for pre, grp in groups:
        for i in range(n_planted // len(groups)):
            p = rnd.choice(grp)
            kind = i % 4
            if kind == 0:
                body = pre
            elif kind == 3:  # near miss in the last byte
                body = p[:-1] + bytes([_other(rnd, p[-1], alpha)])
            else:
                body = p
            a, b = rnd.choice([0, 5, 40]), rnd.choice([0, 7, 60])
            recs.append(_seq(rnd, a, alpha) + body + _seq(rnd, b, alpha))
    recs += [_seq(rnd, 150, alpha) for _ in range(60)]
    rnd.shuffle(recs)
    return raw, recs


def repeats(seed=3, k=31, n_reads=120, long_bytes=200_000):
    """the k-base windows of homopolymers and of period-2 / -3 / -4 repeats, in every phase (a rotation of a unit is a unit).
    Records: microsatellites of 40..600 bases inside random sequence; one record of long_bytes of a period-2 repeat."""
    rnd = random.Random(seed)
    units = [bytes([a]) for a in DNA]
    for period in (2, 3, 4):
        grow = [b""]
        for _ in range(period):
            grow = [u + bytes([a]) for u in grow for a in DNA]
        units += grow
    raw = sorted({(u * k)[:k] for u in units})
    recs = []
    for _ in range(n_reads):
        u = rnd.choice(units)
        n = rnd.randrange(40, 601)
        recs.append(_seq(rnd, rnd.randrange(0, 200)) + (u * n)[:n] + _seq(rnd, rnd.randrange(0, 200)))
    if long_bytes:
        recs.append((b"AC" * (long_bytes // 2 + 1))[:long_bytes])
    return raw, recs


def _same_code(alpha):
    """letter -> the other letters of alpha with the same 2-bit code"""
    return {c: [x for x in alpha if x != c and code2(x) == code2(c)] for c in alpha}


def _respelled(rnd, s, same):
    """s with one to three letters replaced by another letter of the same code: the same keys, another text"""
    v = bytearray(s)
    for k in rnd.sample(range(len(s)), rnd.choice([1, 2, 3])):
        if same.get(v[k]):
            v[k] = rnd.choice(same[v[k]])
    return bytes(v)


def code_collisions(kind="dna", seed=4):
    """a small tiled set plus other spellings of its patterns -- the same 2-bit codes at every place, so the same keys: level
    3 alone tells them apart; the records hold both spellings.
    dna: G -> N, T -> U, A -> Y, C -> R at one to three places of a 31-mer.
    protein: tiled 12-mers of a few protein sequences, 20 letters on 4 codes."""
    rnd = random.Random(seed)
    if kind == "protein":
        raw, recs = tiled(4, 40, 12, seed=seed, n_reads=60, read_len=90, alpha=PROTEIN, flank=30, long_bytes=70_000)
        same = _same_code(PROTEIN)
    else:
        raw, recs = tiled(3, 40, 31, seed=seed, n_reads=60, long_bytes=0)
        same = {ord("G"): [ord("N")], ord("T"): [ord("U")], ord("A"): [ord("Y")], ord("C"): [ord("R")]}
    variants = [_respelled(rnd, p, same) for p in raw[::2]]
    more = [_respelled(rnd, r, same) for r in recs[:120]]  # the other spelling of stretches that hold occurrences
    for v in variants[::3]:  # and the variants themselves, planted
        more.append(_seq(rnd, rnd.randrange(0, 50)) + v + _seq(rnd, rnd.randrange(0, 50)))
    return raw + variants, recs + more


def with_short(raw, records, seed=5, n=None, lengths=(5, 12)):
    """adds one to five short patterns (5..12 bases) cut out of the long ones, so that they occur inside every occurrence
    of the pattern they were cut from"""
    rnd = random.Random(seed)
    shorts = set()
    want = n if n is not None else rnd.randrange(1, 6)
    while len(shorts) < want:
        p = rnd.choice(raw)
        L = rnd.randrange(lengths[0], lengths[1] + 1)
        a = rnd.randrange(0, len(p) - L + 1)
        shorts.add(p[a:a + L])
    return list(raw) + sorted(shorts), list(records)


def mixed_case(records, seed=6):
    """the same records with the case of random letters flipped"""
    rnd = random.Random(seed)
    return [bytes(c ^ 0x20 if rnd.random() < 0.3 and chr(c).isalpha() else c for c in r) for r in records]
