"""Seeded generators of paired input in all four orientations of mem_infer_dir (reference bwamem_pair.c:23-30), shared by
tools/make_orient_fixture.py and the tests: region vectors for the pairing routines (bmh_pestat, bmh_pair, bmh_decide_batch,
bmh_decide_device) and read pairs for mate rescue (bmh_matesw_batch, bmh_matesw_device) and the whole-SAM runs.

The orientations, as mem_infer_dir names them from the first hits' rb (b1, b2) on the doubled coordinate [0, 2 l_pac):
p2 = b2 where both hits lie on one strand, else 2 l_pac - 1 - b2, and
    0 FF  one strand,      p2 >  b1        2 RF  opposite strands, p2 <= b1
    1 FR  opposite strands, p2 >  b1        3 RR  one strand,      p2 <= b1
postgen.py and mswgen.py stay as they are (their fixtures are pinned by seed); they make FR pairs only."""
import numpy as np

import kswgen
import kswlib

FF, FR, RF, RR = range(4)
NAMES = ("FF", "FR", "RF", "RR")
# (mean, standard deviation) of the distance |p2 - b1| per orientation: four windows that differ in position and width
VEC_DISTS = ((300, 40), (400, 60), (2500, 300), (180, 20))
READ_DISTS = ((320, 30), (400, 50), (900, 90), (230, 20))
MIXES = {"all4": (.25, .25, .25, .25), "fr_rf": (0, .6, .4, 0), "ff_rr": (.45, .05, .05, .45)}


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir -> (orientation, distance)"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), abs(p2 - b1)


def _draw_dist(rng, dists, o):
    return max(1, int(round(rng.normal(*dists[o]))))


def paired_vectors4(rng, n_pairs, l_pac, mix, L=150, dists=VEC_DISTS):
    """2 * n_pairs region vectors, shaped like postgen.paired_vectors', and the orientation each pair was placed in.

    The first (best) hits of a pair are placed so that mem_infer_dir gives the orientation o drawn from `mix`, at a distance d
    drawn from dists[o] (one pair in ten: from 4 000-90 000, improper).  With read 1's hit forward at rb = pos:
        FF  read 2 forward,  downstream:  rb = pos + d
        FR  read 2 reverse,  downstream:  rb = 2 l_pac - 1 - (pos + d)
        RF  read 2 reverse,  upstream:    rb = 2 l_pac - 1 - (pos - d)   (read 1 forward and downstream of its mate)
        RR  read 2 forward,  upstream:    rb = pos - d
    Half of the pairs lie wholly on the other strand: both rb moved by l_pac (mod 2 l_pac), which keeps strands' equality, p2 - b1
    and so orientation and distance, and puts read 1 on the reverse strand -- where mem_pair, which names a candidate by the strands
    of the upstream and the downstream hit, files FF under RR's window and the forward RR under FF's.
    Each end then gets 0-6 hits (best score first): the placed hit and further ones at the same forward position on the other
    strand (the mirrored coordinate 2 l_pac - 1 - rb) or 0, 7, 300 or 40 000 bases off on either strand, so that one pair has
    candidates in several orientations and both strands at both ends."""
    out, orient = [], np.zeros(n_pairs, dtype=np.int8)
    two = 2 * l_pac
    for p in range(n_pairs):
        o = int(rng.choice(4, p=mix))
        orient[p] = o
        pos = int(rng.integers(100_000, l_pac - 100_000))
        d = _draw_dist(rng, dists, o) if rng.random() < 0.9 else int(rng.integers(4000, 90000))
        b2 = (pos + d, two - 1 - (pos + d), two - 1 - (pos - d), pos - d)[o]
        base = [pos, b2]
        if rng.random() < 0.5:
            base = [(b + l_pac) % two for b in base]
        assert infer_dir(l_pac, *base) == (o, d)
        for r in range(2):
            n = int(rng.choice([0, 1, 1, 1, 1, 2, 3, 4, 6]))
            a = np.zeros(n, dtype=kswlib.ALNREG)
            for k in range(n):
                rb = base[r]
                if k:
                    if rng.random() < 0.4:
                        rb = two - 1 - rb
                    rb += int(rng.choice([0, 0, 7, -7, 300, -300, 40000]))
                    if rb < l_pac < rb + L:  # a region lies on one strand
                        rb = l_pac
                    rb = min(max(rb, 0), two - L)
                sc = 150 if k == 0 else int(rng.choice([150, 140, 120, 110, 100, 60, 25]))
                a[k]["rb"], a[k]["re"], a[k]["qb"], a[k]["qe"] = rb, rb + L, 0, L
                a[k]["score"], a[k]["truesc"], a[k]["w"], a[k]["seedcov"] = sc, sc, 100, int(rng.integers(19, L))
                a[k]["secondary"] = -1
            # the pairing code expects vectors as mem_mark_primary_se leaves them: best score first (the placed hit stays first)
            out.append(a[np.argsort(-a["score"], kind="stable")])
    return out, orient


def revcomp(s):
    return np.where(s > 3, 4, 3 - s)[::-1].astype(np.uint8)


def read_pairs4(rng, ref, n, L, mix, dists=READ_DISTS, noisy=0.5, noise=0.16):
    """n read pairs (flat, 2 per pair) and their orientations: tools/make_matesw_fixture.sim_pairs with the mate placed in each of
    the four orientations.  The anchor is L lightly mutated bases from ref[pos:]; the mate, at distance d drawn from dists[o], is
        FF  ref[pos + d: pos + d + L]                   FR  the reverse complement of ref[pos + d - L: pos + d]
        RF  the reverse complement of ref[pos - d - L: pos - d]   RR  ref[pos - d: pos - d + L]
    and with probability `noisy` carries substitutions at rate `noise`: too many for a 19-mer seed, only mate rescue places it.
    Either read may be the anchor: in half of the pairs the two change places -- after both were reverse-complemented where the
    orientation is FF or RR, so that mem_infer_dir still gives o, now with read 1 on the reverse strand."""
    reads, orient = [], np.zeros(n, dtype=np.int8)
    span = max(m + 5 * s for m, s in dists) + 2 * L + 80
    for p in range(n):
        o = int(rng.choice(4, p=mix))
        orient[p] = o
        d = _draw_dist(rng, dists, o)
        pos = int(rng.integers(span, len(ref) - span))
        a = kswgen.mutate(rng, ref[pos:pos + L + 30], 0.02, 0.0025, 0.0025, 1)[:L]
        sub = noise if rng.random() < noisy else 0.02
        if o in (FF, RR):
            m0 = pos + d if o == FF else pos - d
            b = kswgen.mutate(rng, ref[m0:m0 + L + 30], sub, 0.004, 0.004, 2)[:L]
        else:
            m1 = pos + d if o == FR else pos - d  # the mate's forward interval ends here
            b = revcomp(kswgen.mutate(rng, ref[m1 - L:m1 + 30], sub, 0.004, 0.004, 2)[:L])
        a, b = a.astype(np.uint8), b.astype(np.uint8)
        if rng.random() < 0.03:
            a[rng.random(len(a)) < 0.03] = 4
        if rng.random() < 0.5:
            a, b = (revcomp(b), revcomp(a)) if o in (FF, RR) else (b, a)
        reads += [a.copy(), b.copy()]
    return reads, orient


def pair_candidates(l_pac, pes, a0, a1):
    """The orientations (as mem_pair names them: strand of the upstream hit << 1 | strand of the downstream hit) in whose window
    some hit of one end and some hit of the other lie -- reference bwamem_pair.c:194-219 restated over all combinations."""
    found = set()
    for x in a0:
        for y in a1:
            hits = sorted(((int(h["rb"]) if int(h["rb"]) < l_pac else 2 * l_pac - 1 - int(h["rb"]), int(h["rb"]) >= l_pac) for h in (x, y)))
            (xk, sk), (xi, si) = hits
            d = sk << 1 | si
            if not int(pes[d]["failed"]) and int(pes[d]["low"]) <= xi - xk <= int(pes[d]["high"]):
                found.add(d)
    return found


def split(flat, counts):
    out, o = [], 0
    for c in counts:
        out.append(flat[o:o + int(c)].copy())
        o += int(c)
    return out


# ---------------------------------------------------------------- the committed fixture (tools/make_orient_fixture.py)

def golden():
    return kswlib.load_golden("orient_golden.npz")


def pairing_groups():
    """Yields (key, option set, mix name, l_pac, vectors, orientations, the reference's table, its mem_pair rows) per pairing group;
    marked_pair_res(key) has the rows over the vectors as mem_mark_primary_se leaves them"""
    g = golden()
    for key in g["pair_groups"]:
        key = str(key)
        si, mix = int(key[1]), key[3:-1]
        yield (key, si, mix, int(g["pair_l_pac"]), split(g[key + "pairs"], g[key + "pairs_n"]), g[key + "orient"],
               np.ascontiguousarray(g[key + "pes"], dtype=kswlib.PESTAT), g[key + "pair_res"])


def pairing_group(key):
    return next(x for x in pairing_groups() if x[0] == key)


def rescue_groups():
    """Yields (key, params, opt, table, l_pac, pac, reads, phase-1 regions, orientations, expected regions, n_sw, mask_level_redun)"""
    g = golden()
    l_pac, pac = int(g["l_pac"]), g["pac"]
    for key in g["rescue_groups"]:
        key = str(key)
        s = key[:key.index("v")] + "_"
        yield (key, g[s + "params"], g[s + "opt"], np.ascontiguousarray(g[key + "pes"], dtype=kswlib.PESTAT), l_pac, pac,
               split(g[s + "reads"], g[s + "read_len"]), split(g[s + "regs"], g[s + "regs_n"]), g[s + "orient"],
               split(g[key + "exp"], g[key + "exp_n"]), g[key + "n_sw"].tolist(), float(g[s + "mask_level_redun"]))



def marked_pair_res(key):
    return golden()[key + "pair_res_marked"]
