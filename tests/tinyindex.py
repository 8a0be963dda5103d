"""A brute-force, bwa-format FM-index of any small forward genome, and the tiny and degenerate genomes the FM-index tests
run on.  bwa indexes the text fwd . revcomp(fwd) (bntseq.c / bwtindex.c: the packed forward strand, then its reverse
complement); here its suffixes are sorted with a plain Python sort and laid out as bwt_bwtupdate_core does (bwtindex.c:
one 64-byte block per 128 symbols, the four running counts before it), with one suffix-array sample per 32 rows
(bwt_cal_sa) and samp[0] = 2^64-1 as `bwa index` leaves it.  tests/test_tiny_index_cpu.py pins the result byte for byte
against `bwa index`."""
import numpy as np

SA_INTV = 32
U64_MAX = 0xffffffffffffffff


def doubled(fwd):
    """bwa's text of a forward genome: codes 0..3, the forward strand and then its reverse complement."""
    fwd = np.asarray(fwd, dtype=np.uint8)
    assert len(fwd) and (fwd < 4).all()
    return np.concatenate([fwd, (3 - fwd[::-1]).astype(np.uint8)])


def build(fwd):
    """-> ((primary, L2, seq_len, bwt words, sa_intv, sa samples), full suffix array).  The first is what make_cbwt /
    set_bwt take; the second has one entry per row 0..seq_len, row 0 being the $ suffix (value seq_len)."""
    T = bytes(doubled(fwd) + 1) + b"\0"
    n = len(T) - 1
    sa = sorted(range(n + 1), key=lambda i: T[i:])
    primary = sa.index(0)
    stream = [T[s - 1] - 1 for k, s in enumerate(sa) if k != primary]  # row 0 is the $ suffix: its symbol is T[n-1]
    L2 = [0]
    for c in range(4):
        L2.append(L2[-1] + stream.count(c))
    words, cnt = [], [0, 0, 0, 0]
    for i in range(n):
        if i % 128 == 0:
            for c in range(4):
                words += [cnt[c] & 0xffffffff, cnt[c] >> 32]
        if i % 16 == 0:
            words.append(0)
        words[-1] |= stream[i] << (30 - 2 * (i % 16))
        cnt[stream[i]] += 1
    for c in range(4):
        words += [cnt[c] & 0xffffffff, cnt[c] >> 32]
    samp = [sa[k] for k in range(0, n + 1, SA_INTV)]
    samp[0] = U64_MAX
    return (primary, L2, n, np.array(words, np.uint32), SA_INTV, np.array(samp, np.uint64)), sa


def sa_rows(sa):
    """What bwt_sa returns for rows 0..seq_len: the suffix array, with row 0 reading the sample `bwa index` overwrites."""
    return np.array([U64_MAX] + list(sa[1:]), dtype=np.uint64)


def _rand(seed, n, lead=()):
    g = np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)
    g[:len(lead)] = lead
    return g


# name -> forward genome (seq_len is twice its length)
SHAPES = {
    "homo_a16": np.zeros(16, np.uint8),                      # text A^16 T^16: primary == 1, C and G absent, one SA sample + 1
    "homo_t16": np.full(16, 3, np.uint8),                    # text T^16 A^16: primary == seq_len
    "homo_c64": np.full(64, 1, np.uint8),                    # text C^64 G^64: L2 = [0, 0, 64, 128, 128], exactly one block
    "ac_63": _rand(21, 63) % 2,                              # A/C only: 126 rows, a partial block and a partial word
    "at_64": (_rand(22, 64) % 2) * 3,                        # A/T only (its own alphabet under complement): 128 rows
    "rand_8": _rand(23, 8),                                  # 16 rows: below one SA sample interval
    "rand_64": _rand(24, 64),                                # 128 rows
    "rand_100": _rand(25, 100),                              # 200 rows: two blocks, the second partial
    "rand_128": _rand(26, 128),                              # 256 rows: exactly two blocks
    "tled_128": _rand(27, 128, lead=(3, 3, 3)),              # 256 rows, the text among the largest suffixes: primary in block 1
    "acg_x50": np.tile(np.array([0, 1, 2], np.uint8), 50),   # 300 rows, period 3
    "rand_1000": _rand(28, 1000),                            # 2000 rows
}

_built = {}


def shape(name):
    """(raw, sa) of a named shape, built once per process."""
    if name not in _built:
        _built[name] = build(SHAPES[name])
    return _built[name]


def absent_bases(raw):
    L2 = raw[1]
    return [c for c in range(4) if L2[c + 1] == L2[c]]


def reads_for(name, n=300):
    """The reads a shape is queried with: every substring of the doubled text when it has 32 rows or fewer; otherwise
    substrings of 1..70 bases with 8 % of the positions redrawn from 0..4 (so that N occurs) and one fifth random
    reads; then one-base reads of every code and reads made of one base only (an absent one among them)."""
    raw, _ = shape(name)
    text = doubled(SHAPES[name])
    rng = np.random.default_rng(len(text) * 131 + len(name))
    out = []
    if len(text) <= 32:
        out = [text[a:b].copy() for a in range(len(text)) for b in range(a + 1, len(text) + 1)]
    else:
        for k in range(n):
            L = int(rng.integers(1, 71))
            if k % 5 == 4:
                out.append(rng.integers(0, 4, L).astype(np.uint8))
                continue
            p = int(rng.integers(0, len(text) - min(L, len(text)) + 1))
            rd = text[p:p + L].copy()
            m = rng.random(len(rd)) < 0.08
            rd[m] = rng.integers(0, 5, int(m.sum()))
            out.append(rd)
    out += [np.array([c], np.uint8) for c in range(5)]
    for c in range(4):  # absent bases are among these
        out += [np.full(L, c, np.uint8) for L in (2, 19, 40)]
    return out
