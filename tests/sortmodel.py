"""A path model of host/sort_exact.h and the inputs that drive it into every path.

bmh_sort_exact_stk (median-of-three quicksort over an explicit range stack, one final insertion sort, combsort once the depth
budget is spent) is restated here in plain Python from that header, with a trace of WHAT RAN: the combsort calls and the size of
each range, the deepest range stack, whether anything beyond the n == 2 exchange or the first partition ran.  The model proves
coverage only -- that a given input sends the C text into a given path.  Expected outputs never come from it: they come from the
compiled reference (tools/make_sort_fixture.py -> tests/golden/sort_paths_golden.npz).

Inputs:
  * McIlroy's adversary ("A Killer Adversary for Quicksort", 1999): keys are "gas" until a comparison has to freeze one; run against
    the model it yields, for a given n, a concrete key sequence on which the quicksort spends its depth budget and calls combsort;
  * deterministic structured orders (ascending, descending, organ-pipe, sawteeth, all-equal, two-valued) and the killer sequences
    with ties folded in (val // 2, val // 8);
  * builders that turn a key sequence into region vectors for mem_sort_and_dedup's two sorts and into one-seed chains (with the
    seeding tables that produce them) for mem_chain_flt's sort.
"""
import zlib

import numpy as np

import kswlib

SIZES = (2, 3, 16, 17, 18, 33, 40, 64, 100, 300, 1000, 2000)
LEVELS = (0.95, 0.8, 0.0, 1.0)  # mask_level_redun


def stack_len(n):
    """bmh_sort_stack_len"""
    k = 2
    while n:
        n >>= 1
        k += 1
    return k


class Trace:
    def __init__(self, n):
        self.n = n
        self.n2 = False         # the n == 2 exchange was all that ran
        self.partitions = []    # size of every range the quicksort partitioned
        self.comb = []          # size of every range handed to combsort
        self.comb_gaps = []     # every gap combsort swept with
        self.max_stack = 0      # deepest range stack
        self.compares = 0

    @property
    def insertion_only(self):
        """nothing ran but the first partition (which every n >= 3 gets) and the final insertion sort over runs of <= 16"""
        return not self.n2 and not self.comb and len(self.partitions) <= 1

    def key(self):
        return (self.n2, tuple(self.partitions), tuple(self.comb), self.max_stack)


def _insertion(a, lt, s, t):
    for i in range(s + 1, t):
        j = i
        while j > s and lt(a[j], a[j - 1]):
            a[j], a[j - 1] = a[j - 1], a[j]
            j -= 1


def _comb(a, lt, s, n, tr):
    shrink = 1.2473309501039786540366528676643
    gap = n
    while True:
        if gap > 2:
            gap = int(float(gap) / shrink)
            if gap == 9 or gap == 10:
                gap = 11
        tr.comb_gaps.append(gap)
        swapped = False
        for i in range(s, s + n - gap):
            if lt(a[i + gap], a[i]):
                a[i], a[i + gap] = a[i + gap], a[i]
                swapped = True
        if not (swapped or gap > 2):
            break
    if gap != 1:
        _insertion(a, lt, s, s + n)


def sort_exact(a, lt):
    """bmh_sort_exact_stk over the list a (in place) with the less-than callable lt.  Returns the Trace."""
    n = len(a)
    tr = Trace(n)
    counted = lt

    def lt(x, y):  # noqa: F811
        tr.compares += 1
        return counted(x, y)

    if n < 1:
        return tr
    if n == 2:
        tr.n2 = True
        if lt(a[1], a[0]):
            a[0], a[1] = a[1], a[0]
        return tr
    d = 2
    while (1 << d) < n:
        d += 1
    stack = []
    s, t, d = 0, n - 1, d << 1
    while True:
        if s < t:
            d -= 1
            if d == 0:  # too deep: combsort the whole range
                tr.comb.append(t - s + 1)
                _comb(a, lt, s, t - s + 1, tr)
                t = s
                continue
            tr.partitions.append(t - s + 1)
            i, j = s, t
            k = i + ((j - i) >> 1) + 1  # median of first, middle+1, last
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            pivot = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], pivot):
                    i += 1
                j -= 1
                while i <= j and lt(pivot, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:  # larger side onto the stack if it is longer than 16, go on with the smaller one
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
            tr.max_stack = max(tr.max_stack, len(stack))
        elif not stack:
            _insertion(a, lt, 0, n)
            return tr
        else:
            s, t, d = stack.pop()


def trace_keys(keys):
    """The model's trace over a sequence of integer keys under plain `<`."""
    a = list(keys)
    tr = sort_exact(a, lambda x, y: x < y)
    assert a == sorted(keys)
    return tr


# ---- McIlroy's adversary --------------------------------------------------------------------------------------------------------

_KILLERS = {}


def killer(n):
    """A permutation of 0..n-1 (as a tuple, in input order) that the adversary froze while the model sorted n items; and the trace of
    that run.  Replaying the frozen values through the model takes the same path (asserted by the tests)."""
    if n in _KILLERS:
        return _KILLERS[n]
    gas = n
    val = [gas] * n
    state = {"solid": 0, "cand": 0}

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            if x == state["cand"]:
                val[x] = state["solid"]
            else:
                val[y] = state["solid"]
            state["solid"] += 1
        if val[x] == gas:
            state["cand"] = x
        elif val[y] == gas:
            state["cand"] = y
        return val[x] < val[y]

    tr = sort_exact(list(range(n)), lt)
    for i in range(n):  # what no comparison had to settle stays largest
        if val[i] == gas:
            val[i] = state["solid"]
            state["solid"] += 1
    assert sorted(val) == list(range(n))
    _KILLERS[n] = (tuple(val), tr)
    return _KILLERS[n]


# ---- key sequences ----------------------------------------------------------------------------------------------------------------

def sequences(n):
    """name -> tuple of n integer keys in 0..n-1, in input order; smaller sorts first."""
    k = killer(n)[0]
    half = (n + 1) // 2
    return {
        "killer": k,
        "killer_div2": tuple(v // 2 for v in k),
        "killer_div8": tuple(v // 8 for v in k),
        "ascending": tuple(range(n)),
        "descending": tuple(range(n - 1, -1, -1)),
        "organ_pipe": tuple(i if i < half else n - 1 - i for i in range(n)),
        "sawtooth3": tuple(i % 3 for i in range(n)),
        "sawtooth17": tuple(i % 17 for i in range(n)),
        "all_equal": (0,) * n,
        "two_valued": tuple((i * 7 // 3) & 1 for i in range(n)),
    }


TIE_FOLDED = ("killer_div2", "killer_div8")


# ---- regions ------------------------------------------------------------------------------------------------------------------------
# Every region carries its input index in seedcov (no routine here reads or writes it), so tied records stay distinguishable and a
# routine's output is its input permuted and thinned: out == in[index list].

ALNREG = kswlib.ALNREG
_R0, _STEP, _LEN = 1_000_000, 1000, 100


def _regs(n):
    a = np.zeros(n, dtype=ALNREG)
    a["w"], a["secondary"] = 100, -1
    a["seedcov"] = np.arange(n)
    return a


def regions_first(keys):
    """First sort (by re): re in input order is the key sequence, `_STEP` apart, each region `_LEN` long, so regions of different
    keys never overlap.  Records of EQUAL key share re and rb (they cannot help overlapping on the reference) and get disjoint query
    intervals instead, so that nothing is redundant at any level and all n reach the second sort.  Scores are distinct."""
    n = len(keys)
    a = _regs(n)
    seen = {}
    for i, k in enumerate(keys):
        j = seen[k] = seen.get(k, -1) + 1
        a[i]["re"] = _R0 + k * _STEP
        a[i]["rb"] = a[i]["re"] - _LEN
        a[i]["qb"], a[i]["qe"] = 2 * _LEN * j, 2 * _LEN * j + _LEN
        a[i]["score"] = a[i]["truesc"] = 20 + (i * 7919) % (n + 13)
    return a


def regions_second(keys):
    """Second sort (bmh_dd_lt_score_pos: the LARGEST score is the smallest record, then rb, then qb).  re is distinct and descending in
    input order, so the first sort leaves the record of rank r at position r whatever it does on ties, and score = top - keys[r]:
    the second sort meets exactly `keys` under its own order.  Records of equal key share (score, rb, qb) -- rb just below the
    smallest re of the group -- and differ in re and qe; groups lie on disjoint query intervals, so only records of one group can be
    redundant.  Those are at every level below 1.0 (the later one in re order survives, equal scores); at 1.0 none is, the ties reach
    the second sort, and the identical-hit pass keeps whichever record that sort put first."""
    n = len(keys)
    a = _regs(n)
    first = {}
    for r, k in enumerate(keys):
        first.setdefault(k, r)
    top = max(keys) + 30 if n else 0
    for i in range(n):
        r = n - 1 - i
        k = keys[r]
        a[i]["re"] = _R0 + r * _STEP
        a[i]["rb"] = _R0 + first[k] * _STEP - _LEN
        a[i]["qb"] = 2 * _LEN * k
        a[i]["qe"] = a[i]["qb"] + _LEN + (r - first[k]) % 50
        a[i]["score"] = a[i]["truesc"] = top - k
    return a


def regions_mixed(keys, fold):
    """Both sorts with masking and compaction between them.  The first sort's key is keys[i] // fold: the records of one group are
    identical but for their index, so below 1.0 each group is redundant throughout and -- scores being equal -- the LAST record in
    the first sort's order survives; at 1.0 all reach the second sort and the identical-hit pass keeps the FIRST in that sort's
    order.  The group's score comes from a killer sequence over the groups (folded by 2, so that equal scores at different rb occur),
    which is what the second sort meets below 1.0."""
    n = len(keys)
    a = _regs(n)
    g = [k // fold for k in keys]
    n_grp = max(g) + 1 if n else 0
    kk = killer(n_grp)[0] if n_grp >= 3 else tuple(range(n_grp))
    for i in range(n):
        a[i]["re"] = _R0 + g[i] * _STEP
        a[i]["rb"] = a[i]["re"] - _LEN
        a[i]["qb"], a[i]["qe"] = 0, _LEN
        a[i]["score"] = a[i]["truesc"] = 30 + n_grp - kk[g[i]] // 2
    return a


def lt_re(x, y):
    return int(x["re"]) < int(y["re"])


def lt_score_pos(x, y):
    a, b = (int(x["score"]), int(x["rb"]), int(x["qb"])), (int(y["score"]), int(y["rb"]), int(y["qb"]))
    return a[0] > b[0] or (a[0] == b[0] and a[1:] < b[1:])


def lt_score_hash(x, y):
    return int(x["score"]) > int(y["score"]) or (int(x["score"]) == int(y["score"]) and int(x["hash"]) < int(y["hash"]))


def trace_mark_sort(survivors, marked):
    """The trace of the sort inside mem_mark_primary_se / bmh_mark_primary_se (score descending, then hash): it meets the survivors
    of de-duplication in their order, each with the hash the routine gave it -- read back from the routine's own output `marked`
    through the index every record carries."""
    h = {int(m["seedcov"]): int(m["hash"]) for m in marked}
    a = [(int(v["score"]), h[int(v["seedcov"])]) for v in survivors]
    return sort_exact(a, lambda x, y: x[0] > y[0] or (x[0] == y[0] and x[1] < y[1]))


MARK_FIELDS = ("seedcov", "secondary", "sub", "sub_n")  # what primary marking decides: the order and these three


def trace_first_sort(vec):
    return sort_exact([vec[i] for i in range(len(vec))], lt_re)


def trace_second_sort_unthinned(vec):
    """The second sort's trace for a vector with distinct re from which the first pass removes nothing (regions_second at level 1.0,
    or with distinct keys at any level): it meets the records in re order."""
    assert len(np.unique(vec["re"])) == len(vec)
    v = vec[np.argsort(vec["re"], kind="stable")]
    return sort_exact([v[i] for i in range(len(v))], lt_score_pos)


# ---- chains -------------------------------------------------------------------------------------------------------------------------
CHAIN_OPT = np.dtype([("w", "<i4"), ("max_chain_gap", "<i4"), ("min_seed_len", "<i4"), ("max_occ", "<i4"), ("split_len", "<i4"),
                      ("split_width", "<i4"), ("mask_level", "<f4"), ("chain_drop_ratio", "<f4")])
# mem_opt_init (reference bwamem.c:45-75), and one set with mask_level and chain_drop_ratio moved
CHAIN_OPTS = (dict(w=100, max_chain_gap=10000, min_seed_len=19, max_occ=10000, split_len=28, split_width=10, mask_level=0.5, chain_drop_ratio=0.5),
              dict(w=100, max_chain_gap=10000, min_seed_len=19, max_occ=10000, split_len=28, split_width=10, mask_level=0.3, chain_drop_ratio=0.7))
CHAIN_L_PAC = 200_000_000
_CH_STEP = 50_000  # further apart than max_chain_gap plus any seed


def chain_opt(kw):
    o = np.zeros((), dtype=CHAIN_OPT)
    for k, v in kw.items():
        o[k] = v
    return o


def chain_seeds(keys):
    """One seed per chain, in reference-position order (the B-tree's read-out order): seed i lies at (i+1)*_CH_STEP on the forward
    strand, so no seed can join another's chain and a chain's weight is its seed's length.  bmh_cc_heavier / flt_lt put the HEAVIER
    chain first, so length = base + (largest key - key): the sort meets `keys` under its own order.  base = n + 19 keeps every
    weight above half the largest, so with the default chain_drop_ratio nothing is dropped and the whole order shows in the output;
    with the ratio moved to 0.7 the light chains go.  Query starts vary a little so that the overlap test sees both outcomes."""
    n = len(keys)
    sd = np.zeros(n, dtype=kswlib.SEED)
    top = max(keys) if n else 0
    for i, k in enumerate(keys):
        sd[i]["rbeg"], sd[i]["qbeg"], sd[i]["len"] = (i + 1) * _CH_STEP, (i % 5) * 3, n + 19 + top - k
    return sd


def chain_read_len(n):
    return 2 * n + 19 + 16  # the longest seed (n + 19 + n - 1) plus the largest query start, and a little


def chain_tables(seeds, opt, base=0):
    """Seeding tables that yield exactly `seeds` for one read: one main call whose intervals are the seeds in order, each with a
    single occurrence; where the longest of them is long and rare enough to have been re-seeded (split_len, split_width),
    smem_next2's order asks for that re-seeding call next -- it found nothing.  base: suffix-array entries of the batch before this
    read; interval k's row is x0 = 1000 + base + k and its position entry base + k.
    Returns (calls, intervals, sa_off, sa_pos)."""
    n = len(seeds)
    intv = np.zeros(n, dtype=kswlib.SMEM_INTV)
    intv["x0"], intv["x1"], intv["x2"] = 1000 + base + np.arange(n), 5000 + np.arange(n), 1
    beg, end = seeds["qbeg"].astype(np.uint64), (seeds["qbeg"] + seeds["len"]).astype(np.uint64)
    intv["info"] = (beg << np.uint64(32)) | end
    calls = np.zeros(1, dtype=kswlib.SMEM_CALL)
    calls[0]["x"], calls[0]["min_intv"], calls[0]["ret"], calls[0]["n"], calls[0]["first"] = 0, 1, 0, n, 0
    if n:
        lens = seeds["len"]
        mi = int(np.argmax(lens))  # the first longest, as smem_next2 takes it
        if int(lens[mi]) >= int(opt["split_len"]) and 1 <= int(opt["split_width"]):
            sc = np.zeros(1, dtype=kswlib.SMEM_CALL)
            sc[0]["x"], sc[0]["min_intv"], sc[0]["n"], sc[0]["first"] = (int(beg[mi]) + int(end[mi])) >> 1, 2, 0, n
            calls = np.concatenate([calls, sc])
        assert int(lens.min()) >= int(opt["min_seed_len"]) and int(end.max()) <= chain_read_len(n)
    return calls, intv, base + np.arange(n, dtype=np.uint64), seeds["rbeg"].astype(np.uint64)


def chain_batch_tables(all_seeds, opt):
    """One read per seed list -> (reads, calls[r], intervals[r], sa_off[r], sa_pos, sa_k): what bmh_chain_batch takes, and the
    sorted row list sa_k with sa_pos[k] the position of row sa_k[k], as tests/test_chain_cpu.py's helpers take it."""
    reads, calls, intvs, offs, pos = [], [], [], [], []
    base = 0
    for sd in all_seeds:
        c, v, o, p = chain_tables(sd, opt, base)
        reads.append(np.zeros(chain_read_len(len(sd)), dtype=np.uint8))
        calls.append(c), intvs.append(v), offs.append(o), pos.append(p)
        base += len(sd)
    sa_pos = np.ascontiguousarray(np.concatenate(pos)) if pos else np.zeros(0, np.uint64)
    return reads, calls, intvs, offs, sa_pos, 1000 + np.arange(len(sa_pos), dtype=np.uint64)


def trace_chain_sort(seeds):
    return sort_exact([int(s["len"]) for s in seeds], lambda x, y: x > y)


# ---- the fixture's cases ------------------------------------------------------------------------------------------------------------
MIXED_MAX = 1000  # records of equal key overlap, and the first pass walks back over their whole group: up to n^2 / 2 steps in one lane
DISTINCT = ("killer", "ascending", "descending")


def first_built(name, n):
    """regions_first: groups of equal key are walked within themselves only, so the tie-folded killers (groups of 2 and 8) stay
    cheap at any size; the orders with few distinct keys stop at MIXED_MAX."""
    return n <= MIXED_MAX or name in DISTINCT or name in TIE_FOLDED


def second_built(name, n):
    """regions_second: a group's records lie scattered over the whole re range and share rb, so the walk crosses everything between
    them; past MIXED_MAX only distinct keys."""
    return n <= MIXED_MAX or name in DISTINCT


def region_cases():
    """(name, vector) of every region case of the fixture, in the fixture's order."""
    out = []
    for n in SIZES:
        for name, keys in sequences(n).items():
            if first_built(name, n):
                out.append((f"first_{name}_{n}", regions_first(keys)))
            if second_built(name, n):
                out.append((f"second_{name}_{n}", regions_second(keys)))
        if n <= MIXED_MAX:
            for fold in (2, 8):
                out.append((f"mixed_div{fold}_{n}", regions_mixed(killer(n)[0], fold)))
    return out


def chain_cases():
    """(name, seeds) of every chain case of the fixture, in the fixture's order."""
    return [(f"chain_{name}_{n}", chain_seeds(keys)) for n in SIZES for name, keys in sequences(n).items()]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---- the fixture ------------------------------------------------------------------------------------------------------------------
_FIXTURE = None


def _cut(flat, cnt):
    at = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return [flat[at[i]: at[i + 1]].astype(np.int64) for i in range(len(cnt))]


def fixture():
    """tests/golden/sort_paths_golden.npz against the cases rebuilt here (names, sizes, sort keys and CRC-32 must agree).  Returns a
    dict: regs = [(name, vector)], reg_want[level] = [the reference's survivors, in its order], reg_marked_crc, chains =
    [(name, seeds)], chain_want[option set] = [the seeds of the chains the reference keeps, in its order]; reg_marked[case] = the MARK_FIELDS columns
    of the reference's primary marking of reg_want[0.95][case], reg_marked_crc[case] the CRC-32 of those records whole."""
    global _FIXTURE
    if _FIXTURE is None:
        import os
        g = np.load(os.path.join(kswlib.GOLDEN_DIR, "sort_paths_golden.npz"))
        assert tuple(g["sizes"]) == SIZES and tuple(np.float32(x) for x in LEVELS) == tuple(g["levels"])
        regs, chains = region_cases(), chain_cases()
        assert [n for n, _ in regs] == [str(x) for x in g["reg_names"]] and [n for n, _ in chains] == [str(x) for x in g["ch_names"]]
        assert (np.concatenate([v["re"] for _, v in regs]) == g["reg_re"]).all() and (np.concatenate([v["score"] for _, v in regs]) == g["reg_score"]).all()
        assert [crc(v) for _, v in regs] == list(g["reg_crc"]), "the builders no longer give the vectors the fixture was made from"
        assert (np.concatenate([s["len"] for _, s in chains]) == g["ch_len"]).all()
        assert [crc(s) for _, s in chains] == list(g["ch_crc"]), "the builders no longer give the chains the fixture was made from"
        f = {"regs": regs, "chains": chains, "reg_marked_crc": g["reg_marked_crc"], "reg_want": {}, "chain_want": []}
        f["reg_marked"] = [np.stack(x, axis=1) if len(x[0]) else np.zeros((0, len(MARK_FIELDS)), np.int64)
                           for x in zip(*[_cut(g["reg_marked_" + k], g["reg_out0_n"]) for k in MARK_FIELDS])]
        for li, level in enumerate(LEVELS):
            f["reg_want"][level] = [v[ix] for (_, v), ix in zip(regs, _cut(g[f"reg_out{li}"], g[f"reg_out{li}_n"]))]
        for oi in range(len(CHAIN_OPTS)):
            f["chain_want"].append([s[ix] for (_, s), ix in zip(chains, _cut(g[f"ch_out{oi}"], g[f"ch_out{oi}_n"]))])
        _FIXTURE = f
    return _FIXTURE
