"""bwa-mem-quickassist_amd -- ctypes binding of libbwamem_hip.so (include/bwamem_hip.h).

The product is the C-ABI shared library built from csrc/ (HIP kernels for gfx950) and
host/ (the batched extension driver, plain C).  This module only loads it and gives the
tests and bench.py a thin, numpy/torch-friendly view of the same entry points; it holds
no algorithmic code and NO fallback: if the library is missing or no GPU is usable,
every call raises.

The directory name is fixed by the project layout and is not a valid Python identifier;
load it with `__graft_entry__.load_package()` (importlib, module name
`bwa_mem_quickassist_amd`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbwamem_hip.so")
DROPIN_PATH = os.path.join(_HERE, "libbwamem_hip_dropin.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "bwamem_hip.h")

BMH_OK, BMH_E_NODEVICE, BMH_E_HIP, BMH_E_ARG, BMH_E_RANGE, BMH_E_NOMEM, BMH_E_CIGAR_CAP = 0, -1, -2, -3, -4, -5, -6
BMH_F_QREV, BMH_F_TREV, BMH_F_TPAC, BMH_F_QCOMP = 1, 2, 4, 8

# record layouts == include/bwamem_hip.h
EXT_TASK = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("qlen", "<u2"), ("tlen", "<u2"),
                     ("h0", "<i4"), ("w", "<i2"), ("end_bonus", "<i2"), ("flags", "<u2"),
                     ("rsv", "<u2")])
EXT_RES = np.dtype([("score", "<i4"), ("qle", "<i4"), ("tle", "<i4"), ("gtle", "<i4"),
                    ("gscore", "<i4"), ("max_off", "<i4")])
SEED_TASK = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("l_query", "<i4"), ("qbeg", "<i4"), ("len", "<i4"),
                      ("rbeg", "<i4"), ("wlen", "<i4"), ("flags", "<u2"), ("rsv", "<u2")])
SEED_RES = np.dtype([("qb", "<i4"), ("qe", "<i4"), ("rb", "<i4"), ("re", "<i4"), ("score", "<i4"), ("truesc", "<i4"),
                     ("w", "<i4"), ("n_ext", "<i4")])
GLB_TASK = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("qlen", "<u2"), ("tlen", "<u2"),
                     ("w", "<i4"), ("cigar_off", "<u4"), ("cigar_cap", "<u4")])
GLB_RES = np.dtype([("score", "<i4"), ("n_cigar", "<i4")])
SW_TASK = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("tlen", "<u4"), ("qlen", "<u2"), ("flags", "<u2"),
                    ("xtra", "<u4"), ("rsv", "<u4")])
SW_RES = np.dtype([("score", "<i4"), ("te", "<i4"), ("qe", "<i4"), ("score2", "<i4"), ("te2", "<i4"),
                   ("tb", "<i4"), ("qb", "<i4"), ("rsv", "<i4")])
KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000  # reference ksw.h:6-9
SMEM_INTV = np.dtype([("x0", "<u8"), ("x1", "<u8"), ("x2", "<u8"), ("info", "<u8")])
SMEM_CALL = np.dtype([("x", "<i4"), ("min_intv", "<i4"), ("ret", "<i4"), ("n", "<i4"), ("first", "<u4"), ("rsv", "<u4")])
SMEM_OPT = np.dtype([("min_seed_len", "<i4"), ("split_len", "<i4"), ("split_width", "<i4"), ("start_width", "<i4"), ("min_emit_len", "<i4")])


class _Bwt(C.Structure):  # bmh_bwt_t
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("bwt_size", C.c_uint64),
                ("bwt", C.c_void_p), ("sa_intv", C.c_int32), ("n_sa", C.c_uint64), ("sa", C.c_void_p)]


PESTAT = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad", "<i4"), ("avg", "<f8"), ("std", "<f8")])
MATESW_OPT = np.dtype([("pen_unpaired", "<i4"), ("max_matesw", "<i4"), ("min_seed_len", "<i4"), ("rsv", "<i4")])
PARAMS = np.dtype([("o_del", "<i4"), ("e_del", "<i4"), ("o_ins", "<i4"), ("e_ins", "<i4"),
                   ("zdrop", "<i4"), ("a", "<i4"), ("w", "<i4"), ("pen_clip5", "<i4"),
                   ("pen_clip3", "<i4"), ("mat", "i1", (25,)), ("pad", "i1", (3,))])
SEED = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])
CIGAR_REQ = np.dtype([("read", "<i4"), ("qb", "<i4"), ("qe", "<i4"), ("pad", "<i4"), ("rb", "<i8"), ("re", "<i8"),
                      ("truesc", "<i4"), ("reg_w", "<i4")])
CIGAR_RES = np.dtype([("score", "<i4"), ("n_cigar", "<i4"), ("NM", "<i4"), ("tries", "<i4"), ("cigar_off", "<u4"),
                      ("md_off", "<u4"), ("md_len", "<u4"), ("rsv", "<u4")])
BMH_REGION_CIGAR_CUT, BMH_REGION_MD_CUT = 1, 2
BMH_REGION_LONG = 4  # finished by the long round of bmh_region_cigar_batch_long
BMH_REGION_LONG_GUARD = 16
REGION_LONG = np.dtype([("region", "<i8"), ("cigar_off", "<u8"), ("md_off", "<u8")])  # 24 bytes
REGION_REQ = np.dtype([("q_src", "<u8"), ("rb", "<i8"), ("o_off", "<u8"), ("ql", "<i4"), ("tl", "<i4"), ("truesc", "<i4"),
                       ("task", "<i4", (3,))])
REGION_RES = np.dtype([("score", "<i4"), ("n_cigar", "<i4"), ("tries", "<i4"), ("NM", "<i4"), ("md_len", "<i4"), ("flags", "<u4")])
SAM_OPT = np.dtype([("a", "<i4"), ("b", "<i4"), ("o_del", "<i4"), ("e_del", "<i4"), ("o_ins", "<i4"), ("e_ins", "<i4"),
                    ("pen_unpaired", "<i4"), ("w", "<i4"), ("T", "<i4"), ("flag", "<i4"), ("min_seed_len", "<i4"), ("max_ins", "<i4"),
                    ("mapQ_coef_fac", "<i4"), ("max_matesw", "<i4"), ("mask_level", "<f4"), ("mask_level_redun", "<f4"),
                    ("mapQ_coef_len", "<f4"), ("mat", "i1", (25,)), ("pad", "i1", (3,))])  # bmh_sam_opt_t
MEM_F_PE, MEM_F_NOPAIRING, MEM_F_ALL = 0x2, 0x4, 0x8
PAIRDEC = np.dtype([("paired", "<i4"), ("z", "<i4", (2,)), ("q_se", "<i4", (2,)), ("extra_flag", "<i4"), ("score", "<i4"), ("sub", "<i4"),
                    ("n_sub", "<i4"), ("q_pe", "<i4"), ("rsv", "<i4", (2,))])  # bmh_pairdec_t
WANTED_RES = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"), ("n_cigar", "<i4"), ("NM", "<i4"),
                       ("tries", "<i4"), ("cigar_off", "<u4"), ("md_off", "<u4"), ("md_len", "<u4"), ("flags", "<u4"), ("band", "<i4", (3,)),
                       ("rsv", "<i4")])  # bmh_wanted_res_t, 72 bytes
PHASE2_STATS = np.dtype([("units", "<i8"), ("wanted", "<i8"), ("fixed", "<i8"), ("redone", "<i8"), ("fallbacks", "<i8"), ("h2d_bytes", "<i8"),
                         ("d2h_bytes", "<i8"), ("waits", "<i4"), ("sessions", "<i4"), ("decide_ms", "<f4"), ("wanted_ms", "<f4")])  # bmh_phase2_stats_t, 72 bytes
SAMTEXT_STATS = np.dtype([("reads", "<i8"), ("lines", "<i8"), ("text_bytes", "<i8"), ("h2d_bytes", "<i8"), ("d2h_bytes", "<i8"), ("waits", "<i4"),
                          ("rsv", "<i4"), ("size_ms", "<f4"), ("emit_ms", "<f4")])  # bmh_samtext_stats_t, 56 bytes
PHASE2_TEXT_STATS = np.dtype([("units", "<i8"), ("wanted", "<i8"), ("fixed", "<i8"), ("redone", "<i8"), ("reads", "<i8"), ("lines", "<i8"),
                              ("text_bytes", "<i8"), ("h2d_bytes", "<i8"), ("d2h_bytes", "<i8"), ("fallbacks", "<i8"), ("waits", "<i4"),
                              ("sessions", "<i4"), ("decide_ms", "<f4"), ("wanted_ms", "<f4"), ("gather_ms", "<f4"), ("size_ms", "<f4"),
                              ("emit_ms", "<f4"), ("rsv", "<i4")])  # bmh_phase2_text_stats_t, 112 bytes
READS_SAM_STATS = np.dtype([("reads", "<i8"), ("regions_in", "<i8"), ("regions", "<i8"), ("kmax", "<i8"), ("opool_cap", "<i8"),
                            ("handoff_d2h_bytes", "<i8"), ("waits_tail", "<i4"), ("plan_ms", "<f4"), ("neg_index", "<i4"),
                            ("rsv", "<i4")])  # bmh_reads_sam_stats_t, 64 bytes
PAIRS_SAM_STATS = np.dtype([("reads", "<i8"), ("pairs", "<i8"), ("regions_in", "<i8"), ("regions", "<i8"), ("regions_out", "<i8"), ("n_sw", "<i8"),
                            ("kmax", "<i8"), ("pair_kmax", "<i8"), ("opool_cap", "<i8"), ("mid_d2h_bytes", "<i8"), ("mid_h2d_bytes", "<i8"),
                            ("waits_mid", "<i4"), ("pes_given", "<i4"), ("plan_ms", "<f4"), ("neg_index", "<i4"),
                            ("rsv", "<i4", (6,))])  # bmh_pairs_sam_stats_t, 128 bytes
PAIRS_PARKED_INFO = np.dtype([("device", "<i4"), ("reads", "<i4"), ("regions", "<i8"), ("bytes", "<i8")])  # bmh_pairs_parked_info_t, 24 bytes
MATESW_TABLE_STATS = np.dtype([("regions_in", "<i8"), ("regions_out", "<i8"), ("arena_records", "<i8"), ("hits", "<i8"), ("mid_bytes", "<i8"),
                               ("pairs", "<i4"), ("active", "<i4"), ("waits", "<i4"), ("filter_ms", "<f4"), ("pack_ms", "<f4"),
                               ("merge_ms", "<f4")])  # bmh_matesw_table_stats_t, 64 bytes
WANTED_MOVED, WANTED_HOST = 4, 8
MEM_F_NO_MULTI = 0x10
MEM_F_NO_EXACT = 0x40
ALNREG = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("score", "<i4"),
                   ("truesc", "<i4"), ("sub", "<i4"), ("csub", "<i4"), ("sub_n", "<i4"),
                   ("w", "<i4"), ("seedcov", "<i4"), ("secondary", "<i4"), ("hash", "<u8")])


class BmhError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        super().__init__(f"libbwamem_hip error {code}: {detail}")


class _Chain(C.Structure):
    _fields_ = [("n", C.c_int32), ("m", C.c_int32), ("pos", C.c_int64), ("seeds", C.c_void_p)]


class _ChainV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.POINTER(_Chain))]


class _AlnregV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class _Read(C.Structure):
    _fields_ = [("l_seq", C.c_int32), ("seq", C.c_void_p)]


class _Seq(C.Structure):  # bmh_seq_t
    _fields_ = [("l_seq", C.c_int32), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


class _RefAnn(C.Structure):  # bmh_refann_t
    _fields_ = [("offset", C.c_int64), ("len", C.c_int32), ("n_ambs", C.c_int32), ("gi", C.c_uint32), ("name", C.c_char_p), ("anno", C.c_char_p)]


class _RefIdx(C.Structure):  # bmh_refidx_t
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seed", C.c_uint32), ("anns", C.POINTER(_RefAnn))]


def make_refidx(contigs, l_pac=None, names=None):
    """bmh_refidx_t over contigs = [(offset, len), ...] (names seq0, seq1, ... unless given); l_pac defaults to the end of the last one."""
    anns = (_RefAnn * max(len(contigs), 1))()
    for i, (off, ln) in enumerate(contigs):
        anns[i] = _RefAnn(int(off), int(ln), 0, 0, names[i] if names is not None else b"seq%d" % i, b"")
    idx = _RefIdx(int(l_pac if l_pac is not None else contigs[-1][0] + contigs[-1][1]), len(contigs), 11, anns)
    idx._keep = anns
    return idx


class _ChainStats(C.Structure):  # bmh_chain_stats_t
    _fields_ = [("reads", C.c_int64), ("chains_in", C.c_int64), ("chains_out", C.c_int64), ("seeds", C.c_int64), ("equal_keys", C.c_int64),
                ("kernel_ms", C.c_float)]


CHAIN_OPT = np.dtype([("w", "<i4"), ("max_chain_gap", "<i4"), ("min_seed_len", "<i4"), ("max_occ", "<i4"), ("split_len", "<i4"),
                      ("split_width", "<i4"), ("mask_level", "<f4"), ("chain_drop_ratio", "<f4")])


def _take_chains(out, n):
    """bmh_chain_v[n] -> per read a list of SEED arrays in chain order; frees the C allocations."""
    res = []
    for k in range(n):
        chains = []
        for ci in range(out[k].n):
            c = out[k].a[ci]
            sd = np.zeros(c.n, dtype=SEED)
            if c.n:
                C.memmove(sd.ctypes.data, c.seeds, c.n * SEED.itemsize)
            chains.append(sd)
            _libc.free(c.seeds)
        if out[k].a:
            _libc.free(C.cast(out[k].a, C.c_void_p))
        res.append(chains)
    return res


class _DriverStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("rounds", "ext_tasks", "seeds_extended", "seeds_skipped", "pool_bytes", "seeds_speculated", "short_sw")]


_lib = None


def lib():
    """The loaded C-ABI library.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BmhError(BMH_E_NODEVICE, f"{LIB_PATH} not built; run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        L.bmh_strerror.restype = C.c_char_p
        L.bmh_last_error.restype = C.c_char_p
        L.bmh_last_error.argtypes = [C.c_void_p]
        for name in ("bmh_ctx_destroy", "bmh_ctx_sync"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.bmh_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.bmh_ctx_set_params.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_qcap.argtypes = [C.c_void_p, C.c_int]
        L.bmh_ctx_set_wide_extension.argtypes = [C.c_void_p, C.c_int]
        L.bmh_extend_wide_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_global_long_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_ctx_set_wide_sw.argtypes = [C.c_void_p, C.c_int]
        L.bmh_sw_wide_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_ctx_reserve_staging.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
        L.bmh_ctx_reserve_device.argtypes = [C.c_void_p, C.c_size_t, C.c_int64, C.c_size_t]
        L.bmh_ctx_reserve_kernels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int]
        L.bmh_ctx_set_pac.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bmh_set_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.bmh_last_extend_bin_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.bmh_last_global_bin_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.bmh_last_global_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bmh_last_global_bin_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_extend_rows.argtypes = [C.c_void_p, C.c_int64]
        L.bmh_last_extend_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bmh_last_extend_bands.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bmh_last_seedext_round_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.bmh_extend_bin_ms_sum.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]
        L.bmh_upload_pool.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.bmh_extend_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_extend_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.bmh_seedext_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_seedext_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_seedext_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.bmh_seedext_wait.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_seedext_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_bwt.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_smem_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_size_t]
        L.bmh_sa_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_chain_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.bmh_seed_chain_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.bmh_chain_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_matesw_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmh_matesw_device.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p]
        L.bmh_matesw_table_device.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmh_last_matesw_table_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_sw_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_sw_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.bmh_extend_batch_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_int64, C.c_void_p]
        L.bmh_global_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_size_t]
        L.bmh_global_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
        L.bmh_chain2aln_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmh_driver_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_chains2regs_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bmh_chains2regs_device.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bmh_seed_chain_regs_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.bmh_sort_dedup_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float]
        L.bmh_ctx_set_regs_dedup.argtypes = [C.c_void_p, C.c_int, C.c_float]
        L.bmh_last_dedup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_pestat_candidates.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.bmh_pestat_from_candidates.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
        L.bmh_pestat_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_regs_drop_exact.argtypes = [C.c_void_p, C.c_int]
        L.bmh_ctx_set_pestat_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.bmh_last_pestat_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
        L.bmh_last_drop_exact_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.bmh_decide_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 6
        L.bmh_decide_device.argtypes = [C.c_void_p] + L.bmh_decide_batch.argtypes
        L.bmh_ctx_set_decide_device.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_decide_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_wanted_cigar_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p, C.c_size_t]
        L.bmh_wanted_cigar_device.argtypes = L.bmh_wanted_cigar_batch.argtypes
        L.bmh_ctx_set_refidx.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_wanted_device.argtypes = [C.c_void_p, C.c_int]
        L.bmh_phase2_device.argtypes = ([C.c_void_p] * 5 + [C.c_int64, C.c_int] + [C.c_void_p] * 8 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t])
        L.bmh_ctx_set_phase2_device.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_phase2_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_sam_text_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_char_p, C.c_void_p, C.c_void_p]
        L.bmh_sam_text_device.argtypes = [C.c_void_p] + L.bmh_sam_text_batch.argtypes
        L.bmh_ctx_set_refnames.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_samtext_device.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_samtext_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_phase2_text_device.argtypes = [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
        L.bmh_ctx_set_phase2_text_device.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_phase2_text_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_reads_sam_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
        L.bmh_last_reads_sam_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_pairs_sam_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
        L.bmh_last_pairs_sam_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_pairs_sam_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmh_pairs_sam_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p]
        L.bmh_pairs_finish_consumed.argtypes = [C.c_void_p]
        L.bmh_pairs_parked_free.argtypes = [C.c_void_p]
        L.bmh_pairs_parked_free.restype = None
        L.bmh_pairs_parked_info.argtypes = [C.c_void_p, C.c_void_p]
        L.bmh_pairs_parked_trim.argtypes = [C.c_int]
        L.bmh_last_wanted_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_region_cigar_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bmh_region_cigar_batch.restype = C.c_int
        L.bmh_region_cigar_batch_long.argtypes = L.bmh_region_cigar_batch.argtypes + [C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.bmh_region_cigar_batch_long.restype = C.c_int
        L.bmh_last_region_long_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        L.bmh_ctx_set_region_long.argtypes = [C.c_void_p, C.c_int]
        L.bmh_last_reg2cigar_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.bmh_reg2cigar_batch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        _lib = L
    return _lib


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _nbytes(a):
    return a.nbytes if a is not None else 0


class ParkedPairs:
    """What bmh_pairs_sam_begin parked (bmh_pairs_parked_t): Context.pairs_sam_finish consumes it, free() gives its block back unfinished."""

    def __init__(self, h):
        self._h = h

    def info(self):
        """bmh_pairs_parked_info as a dict: device, reads, regions, bytes"""
        st = np.zeros(1, dtype=PAIRS_PARKED_INFO)
        rc = lib().bmh_pairs_parked_info(self._h, _ptr(st))
        if rc:
            raise BmhError(rc, lib().bmh_strerror(rc).decode())
        return {k: st[0][k].item() for k in PAIRS_PARKED_INFO.names}

    def free(self):
        if self._h:
            lib().bmh_pairs_parked_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pairs_parked_trim(device=0):
    """bmh_pairs_parked_trim: the idle parked blocks of `device` go back to the runtime"""
    rc = lib().bmh_pairs_parked_trim(int(device))
    if rc:
        raise BmhError(rc, lib().bmh_strerror(rc).decode())


class Context:
    """One GPU + one stream (bmh_ctx_t).  Mirrors the C-ABI one to one."""

    def __init__(self, device=0, params=None):
        self._h = C.c_void_p()
        rc = lib().bmh_ctx_create(C.byref(self._h), int(device))
        if rc:
            raise BmhError(rc, lib().bmh_strerror(rc).decode())
        if params is not None:
            self.set_params(params)

    def _check(self, rc):
        if rc:
            raise BmhError(rc, f"{lib().bmh_strerror(rc).decode()}: {lib().bmh_last_error(self._h).decode()}")

    def close(self):
        if self._h:
            lib().bmh_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, p):
        p = np.ascontiguousarray(np.asarray(p, dtype=PARAMS).reshape(()))
        self._check(lib().bmh_ctx_set_params(self._h, _ptr(p)))

    def set_stream(self, hip_stream_ptr):
        self._check(lib().bmh_ctx_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_pac(self, pac, l_pac):
        """Make the 2-bit reference resident on the device (BMH_F_TPAC tasks; drivers skip the host bns_get_seq).
        The array is kept alive and must be passed unchanged to the drivers (they recognise it by address)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        self._pac = pac
        self._check(lib().bmh_ctx_set_pac(self._h, _ptr(pac), int(l_pac)))
        return pac

    def set_qcap(self, q):
        self._check(lib().bmh_ctx_set_qcap(self._h, int(q)))

    def set_wide_extension(self, on=True):
        """Opt in to the int32 extension kernel: scores past 32000, queries past 13 632 and gap costs past 16 bits go to it
        instead of being refused (bmh_ctx_set_wide_extension)."""
        self._check(lib().bmh_ctx_set_wide_extension(self._h, 1 if on else 0))

    def extend_wide_stats(self):
        """(tasks, ms) the last extension launch sent to the int32 kernel; ms is -1 with timing off (bmh_extend_wide_stats)."""
        n, ms = C.c_int64(0), C.c_float(-1)
        self._check(lib().bmh_extend_wide_stats(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def global_long_stats(self):
        """(tasks, ms) this context's global-alignment launches have sent to the band-ring kernel so far (queries past 10 176
        columns); ms sums its kernel time over the launches made with timing on, -1 with timing off (bmh_global_long_stats)."""
        n, ms = C.c_int64(0), C.c_float(-1)
        self._check(lib().bmh_global_long_stats(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def set_wide_sw(self, on=True):
        """Opt in to the long-query Smith-Waterman kernel: word-mode ksw_align2 tasks past qlen*max(mat) >= 32000 are accepted
        (saturating as the reference does), and every word-mode task the slab kernel would take runs on one wave per task
        (bmh_ctx_set_wide_sw)."""
        self._check(lib().bmh_ctx_set_wide_sw(self._h, 1 if on else 0))

    def sw_wide_stats(self):
        """(tasks, ms) this context's Smith-Waterman launches have sent to the long-query kernel so far; ms sums its kernel time
        over the launches made with timing on, -1 with timing off (bmh_sw_wide_stats)."""
        n, ms = C.c_int64(0), C.c_float(-1)
        self._check(lib().bmh_sw_wide_stats(self._h, C.byref(n), C.byref(ms)))
        return int(n.value), float(ms.value)

    def reserve_staging(self, upload_bytes, download_bytes):
        """Pinned staging buffers of the host-buffer entry points, allocated ahead of the first batch."""
        self._check(lib().bmh_ctx_reserve_staging(self._h, int(upload_bytes), int(download_bytes)))

    def reserve_device(self, pool_bytes, max_tasks, cigar_words):
        """Device workspaces of the host-buffer entry points, allocated ahead of the first batch (bmh_ctx_reserve_device)."""
        self._check(lib().bmh_ctx_reserve_device(self._h, int(pool_bytes), int(max_tasks), int(cigar_words)))

    def reserve_kernels(self, seed_reads, seed_read_len, global_tasks, global_rows):
        """Kernel scratch of the SMEM and global lane kernels, allocated ahead of the first batch (bmh_ctx_reserve_kernels)."""
        self._check(lib().bmh_ctx_reserve_kernels(self._h, int(seed_reads), int(seed_read_len), int(global_tasks), int(global_rows)))

    def sync(self):
        self._check(lib().bmh_ctx_sync(self._h))

    def set_kernel_timing(self, on=True):
        self._check(lib().bmh_set_kernel_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self):
        ms = C.c_float(-1)
        self._check(lib().bmh_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_extend_bin_ms(self):
        ms = (C.c_float * 6)()
        self._check(lib().bmh_last_extend_bin_ms(self._h, ms))
        return [float(x) for x in ms]

    def extend_bin_ms_sum(self, reset=True):
        """per-bin kernel time summed over the dispatcher launches since the last reset (timing mode) -> (ms[6], launches)"""
        ms = (C.c_double * 6)()
        n = C.c_longlong(0)
        self._check(lib().bmh_extend_bin_ms_sum(self._h, ms, C.byref(n), 1 if reset else 0))
        return [float(x) for x in ms], int(n.value)

    def last_seedext_round_ms(self):
        ms = (C.c_float * 4)()
        self._check(lib().bmh_last_seedext_round_ms(self._h, ms))
        return [float(x) for x in ms]

    def last_global_bin_ms(self):
        ms = (C.c_float * 3)()
        self._check(lib().bmh_last_global_bin_ms(self._h, ms))
        return [float(x) for x in ms]

    def last_global_bands(self, n):
        """Diagnostic: the band the device computed for each of the n tasks of the most recent global launch, by input position
        (uint8, 255 = wider than 254).  Raises when that launch ran no band pass or had another task count (bmh_last_global_bands)."""
        bands = np.zeros(int(n), dtype=np.uint8)
        self._check(lib().bmh_last_global_bands(self._h, _ptr(bands), int(n)))
        return bands

    def last_global_bin_counts(self):
        """Diagnostic: the tasks of the most recent global launch per dispatcher bin (uint32 x 8; bins 6 and 7 are the exact-band
        kernel's).  Raises once a later call has sorted tasks of its own (bmh_last_global_bin_counts)."""
        counts = np.zeros(8, dtype=np.uint32)
        self._check(lib().bmh_last_global_bin_counts(self._h, _ptr(counts)))
        return counts

    def set_extend_rows(self, cap):
        """Diagnostic: plain extension launches record the rows each lane-kernel task ran, for task indices below cap; 0 turns it
        off (bmh_ctx_set_extend_rows)."""
        self._check(lib().bmh_ctx_set_extend_rows(self._h, int(cap)))

    def last_extend_rows(self, n):
        """The rows tasks 0..n-1 of the most recent plain extension launch ran, by task index (uint16; 0xffff: no lane kernel took
        the task).  Raises when nothing was recorded or n is past the launch's cap (bmh_last_extend_rows)."""
        rows = np.zeros(int(n), dtype=np.uint16)
        self._check(lib().bmh_last_extend_rows(self._h, _ptr(rows), int(n)))
        return rows

    def last_extend_bands(self, n):
        """Diagnostic: the band each of the n entries of the most recent extension launch with a band pass was run on, by input
        position (uint8; 255 = the task's own, 255 or wider).  Raises when that launch had no band pass or another entry count
        (bmh_last_extend_bands)."""
        bands = np.zeros(int(n), dtype=np.uint8)
        self._check(lib().bmh_last_extend_bands(self._h, _ptr(bands), int(n)))
        return bands

    # ---- L2, host buffers
    def upload_pool(self, pool):
        """Leave a sequence pool resident on the device (bmh_upload_pool): extend_batch / global_batch / seedext_batch with
        pool=None and seedext_submit run against it."""
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        self._check(lib().bmh_upload_pool(self._h, _ptr(pool), pool.nbytes))

    def extend_batch(self, pool, tasks):
        """N x ksw_extend2 (reference ksw.c:379).  numpy in, numpy out; pool=None: the pool left by upload_pool()."""
        pool = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint8)
        tasks = np.ascontiguousarray(tasks, dtype=EXT_TASK)
        res = np.zeros(len(tasks), dtype=EXT_RES)
        self._check(lib().bmh_extend_batch(self._h, _ptr(pool), _nbytes(pool), _ptr(tasks), len(tasks), _ptr(res)))
        return res

    def seedext_batch(self, pool, tasks):
        """N x (left extension, clip decision, right extension from the left score): the fused per-seed record
        (reference bwamem.c:810-866; ext_param_t / ext_res_t :553-577).  numpy in, numpy out; pool=None: the pool left by
        upload_pool()."""
        pool = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint8)
        tasks = np.ascontiguousarray(tasks, dtype=SEED_TASK)
        res = np.zeros(len(tasks), dtype=SEED_RES)
        self._check(lib().bmh_seedext_batch(self._h, _ptr(pool), _nbytes(pool), _ptr(tasks), len(tasks), _ptr(res)))
        return res

    def seedext_submit(self, tasks):
        """First half of the two-step fused per-seed call (bmh_seedext_submit): stages the seeds and enqueues everything
        against the pool left by upload_pool(), then returns; seedext_wait() delivers the records."""
        tasks = np.ascontiguousarray(tasks, dtype=SEED_TASK)
        self._check(lib().bmh_seedext_submit(self._h, _ptr(tasks), len(tasks)))
        self._seed_pending = len(tasks)

    def seedext_wait(self):
        """Second half (bmh_seedext_wait): blocks until the submitted seeds' records are there and returns them."""
        n, self._seed_pending = getattr(self, "_seed_pending", None) or 0, None
        res = np.zeros(n, dtype=SEED_RES)
        self._check(lib().bmh_seedext_wait(self._h, _ptr(res) if n else None))
        return res

    def seedext_batch_device(self, d_pool, d_tasks, n, d_res):
        self._check(lib().bmh_seedext_batch_device(self._h, C.c_void_p(d_pool), C.c_void_p(d_tasks), int(n), C.c_void_p(d_res)))

    def seedext_stats(self):
        st = (C.c_int64 * 5)()
        self._check(lib().bmh_seedext_stats(self._h, st))
        return dict(zip(("seeds", "left_tasks", "left_retries", "right_tasks", "right_retries"), [int(x) for x in st]))

    def global_batch(self, pool, tasks, cigar_words):
        """N x ksw_global2 (reference ksw.c:501).  Returns (results, cigar_pool); pool=None: the pool left by upload_pool()."""
        pool = None if pool is None else np.ascontiguousarray(pool, dtype=np.uint8)
        tasks = np.ascontiguousarray(tasks, dtype=GLB_TASK)
        res = np.zeros(len(tasks), dtype=GLB_RES)
        cig = np.zeros(max(int(cigar_words), 1), dtype=np.uint32)
        self._check(lib().bmh_global_batch(self._h, _ptr(pool), _nbytes(pool), _ptr(tasks), len(tasks), _ptr(res),
                                           _ptr(cig), int(cigar_words)))
        return res, cig

    def region_cigar_batch(self, readpool, opool_bytes, reqs, tasks, task_cigar_words, cig_cap=24, md_cap=64):
        """One record per region: bwa_gen_cigar2's byte work around ksw_global2 on the device (reference bwa.c:89-172, bwamem.c:1194-1201);
        needs set_pac().  Returns (results, cigar words [n, cig_cap], MD bytes [n, md_cap])."""
        readpool = np.ascontiguousarray(readpool, dtype=np.uint8)
        reqs = np.ascontiguousarray(reqs, dtype=REGION_REQ)
        tasks = np.ascontiguousarray(tasks, dtype=GLB_TASK)
        res = np.zeros(len(reqs), dtype=REGION_RES)
        cig = np.zeros((max(len(reqs), 1), cig_cap), dtype=np.uint32)
        md = np.zeros((max(len(reqs), 1), md_cap), dtype=np.uint8)
        self._check(lib().bmh_region_cigar_batch(self._h, _ptr(readpool), readpool.nbytes, int(opool_bytes), _ptr(reqs), len(reqs),
                                                 _ptr(tasks), len(tasks), int(task_cigar_words), int(cig_cap), int(md_cap), _ptr(res),
                                                 _ptr(cig), _ptr(md)))
        return res, cig, md

    def region_cigar_batch_long(self, readpool, opool_bytes, reqs, tasks, task_cigar_words, cig_cap=24, md_cap=64, guard=0):
        """region_cigar_batch() with the regions past their slots finished on the device (bmh_region_cigar_batch_long).  Returns
        (results, cigar words [n, cig_cap], MD bytes [n, md_cap], longs, long_cigar, long_md): longs is a REGION_LONG array, ascending
        by region, into the two dense pools -- copies, the call's own allocations are freed here.  guard: bytes behind each of the
        three outputs the call is given that must come back untouched (checked here; a test's knob)."""
        readpool = np.ascontiguousarray(readpool, dtype=np.uint8)
        reqs = np.ascontiguousarray(reqs, dtype=REGION_REQ)
        tasks = np.ascontiguousarray(tasks, dtype=GLB_TASK)
        n = len(reqs)
        res_b = np.full(n * REGION_RES.itemsize + guard + 1, 0x5A, dtype=np.uint8)
        cig_b = np.full(max(n, 1) * cig_cap * 4 + guard, 0x5A, dtype=np.uint8)
        md_b = np.full(max(n, 1) * md_cap + guard, 0x5A, dtype=np.uint8)
        longs, n_long, lcig, lmd = C.c_void_p(), C.c_int64(-1), C.c_void_p(), C.c_void_p()
        self._check(lib().bmh_region_cigar_batch_long(self._h, _ptr(readpool), readpool.nbytes, int(opool_bytes), _ptr(reqs), n, _ptr(tasks),
                                                      len(tasks), int(task_cigar_words), int(cig_cap), int(md_cap), _ptr(res_b), _ptr(cig_b),
                                                      _ptr(md_b), C.byref(longs), C.byref(n_long), C.byref(lcig), C.byref(lmd)))
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        try:
            res = res_b[:n * REGION_RES.itemsize].view(REGION_RES).copy()
            assert (res_b[n * REGION_RES.itemsize:] == 0x5A).all() and (cig_b[max(n, 1) * cig_cap * 4:] == 0x5A).all() \
                and (md_b[max(n, 1) * md_cap:] == 0x5A).all(), "bmh_region_cigar_batch_long wrote behind one of its outputs"
            cig = cig_b[:max(n, 1) * cig_cap * 4].view(np.uint32).reshape(max(n, 1), cig_cap).copy()
            md = md_b[:max(n, 1) * md_cap].reshape(max(n, 1), md_cap).copy()
            nl = n_long.value
            lg = np.zeros(nl, dtype=REGION_LONG)
            lc, lm = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
            if nl > 0:
                C.memmove(lg.ctypes.data, longs.value, nl * REGION_LONG.itemsize)
                fl = res[lg["region"]]
                words = int((lg["cigar_off"] + fl["n_cigar"].astype(np.uint64)).max())
                mbytes = int((lg["md_off"] + fl["md_len"].astype(np.uint64)).max())
                lc, lm = np.zeros(words, dtype=np.uint32), np.zeros(mbytes, dtype=np.uint8)
                C.memmove(lc.ctypes.data, lcig.value, words * 4)
                C.memmove(lm.ctypes.data, lmd.value, mbytes)
                # the pools are dense and end with their last entry; behind each come BMH_REGION_LONG_GUARD bytes of 0xA5, set on the
                # device before the kernels ran and brought back with the pool
                g = np.zeros(2 * BMH_REGION_LONG_GUARD, dtype=np.uint8)
                C.memmove(g.ctypes.data, lcig.value + words * 4, BMH_REGION_LONG_GUARD)
                C.memmove(g.ctypes.data + BMH_REGION_LONG_GUARD, lmd.value + mbytes, BMH_REGION_LONG_GUARD)
                assert (g == 0xA5).all(), "the long round wrote behind one of its pools"
        finally:
            libc.free(longs), libc.free(lcig), libc.free(lmd)
        return res, cig, md, lg, lc, lm

    def last_region_long_stats(self):
        """bmh_last_region_long_stats: (regions, cigar_words, md_bytes, kernel_ms) of the last region_cigar_batch_long()."""
        a, b, c, ms = C.c_int64(), C.c_int64(), C.c_int64(), C.c_float()
        self._check(lib().bmh_last_region_long_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)))
        return a.value, b.value, c.value, ms.value

    def set_region_long(self, on=True):
        """bmh_ctx_set_region_long: while on, reg2cigar_batch() -- and pass B of phase 2 through it -- finishes the regions past the
        region record's slots on the device instead of redoing them with host copies."""
        self._check(lib().bmh_ctx_set_region_long(self._h, 1 if on else 0))

    def last_reg2cigar_stats(self):
        """bmh_last_reg2cigar_stats: (regions, long_device, redone_host) of the last reg2cigar_batch() on this context."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(lib().bmh_last_reg2cigar_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- L2, device-resident (raw device pointers, e.g. torch tensors' data_ptr())
    def sw_batch(self, pool, tasks):
        """N x ksw_align2 (reference ksw.c:341; mate rescue / short chains).  numpy in, numpy out (kswr_t fields)."""
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        tasks = np.ascontiguousarray(tasks, dtype=SW_TASK)
        res = np.zeros(len(tasks), dtype=SW_RES)
        self._check(lib().bmh_sw_batch(self._h, _ptr(pool), pool.nbytes, _ptr(tasks), len(tasks), _ptr(res)))
        return res

    def sw_batch_device(self, d_pool, d_tasks, n, d_res):
        self._check(lib().bmh_sw_batch_device(self._h, C.c_void_p(d_pool), C.c_void_p(d_tasks), int(n), C.c_void_p(d_res)))

    def set_bwt(self, primary, L2, seq_len, bwt_words, sa_intv, sa):
        """Make the FM-index resident (the arrays of the reference's bwt_t, bwt.h:45-57)."""
        bw = np.ascontiguousarray(bwt_words, dtype=np.uint32)
        sa = np.ascontiguousarray(sa, dtype=np.uint64)
        self._bwt_keep = (bw, sa)
        b = _Bwt()
        b.primary, b.seq_len, b.bwt_size, b.sa_intv, b.n_sa = int(primary), int(seq_len), len(bw), int(sa_intv), len(sa)
        for i in range(5):
            b.L2[i] = int(L2[i])
        b.bwt, b.sa = bw.ctypes.data, sa.ctypes.data
        self._check(lib().bmh_ctx_set_bwt(self._h, C.byref(b)))

    def smem_batch(self, opt, reads):
        """The bwt_smem1 calls of smem_next2's iteration for every read (reference bwt.c:288, bwamem.c:118).
        Returns per read (SMEM_CALL[], SMEM_INTV[])."""
        n = len(reads)
        o_in, opt = np.asarray(opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:  # (records written before a field existed leave it 0)
            opt[k] = o_in[k]
        keep = []
        c_reads = (_Read * max(n, 1))()
        tot = 0
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
            tot += len(r)
        call_cap, intv_cap = tot // 4 + 64 * n + 64, 2 * tot + 1024
        call_off = np.zeros(n + 1, dtype=np.uint32)
        intv_off = np.zeros(n + 1, dtype=np.uint64)
        while True:
            calls = np.zeros(call_cap, dtype=SMEM_CALL)
            intv = np.zeros(intv_cap, dtype=SMEM_INTV)
            rc = lib().bmh_smem_batch(self._h, _ptr(opt), n, C.cast(c_reads, C.c_void_p), _ptr(call_off), _ptr(calls),
                                      C.c_size_t(call_cap), _ptr(intv_off), _ptr(intv), C.c_size_t(intv_cap))
            if rc != BMH_E_CIGAR_CAP:
                break
            call_cap, intv_cap = 2 * call_cap, 4 * intv_cap  # totals are data dependent: grow and ask again
        self._check(rc)
        out = []
        for r in range(n):
            out.append((calls[call_off[r]:call_off[r + 1]].copy(), intv[int(intv_off[r]):int(intv_off[r + 1])].copy()))
        return out

    def seed_batch(self, opt, max_occ, reads):
        """bmh_seed_batch: smem_batch plus, per interval, where its suffix-array positions start (sa_off, UINT64_MAX = not
        looked up) and the positions.  Returns (per-read [(calls, intervals)], per-read sa_off arrays, sa_pos)."""
        n = len(reads)
        o_in, opt = np.asarray(opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            opt[k] = o_in[k]
        keep = []
        c_reads = (_Read * max(n, 1))()
        tot = 0
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
            tot += len(r)
        call_cap, intv_cap, sa_cap = tot // 4 + 64 * n + 64, 2 * tot + 1024, 4 * tot + 4096
        call_off = np.zeros(n + 1, dtype=np.uint32)
        intv_off = np.zeros(n + 1, dtype=np.uint64)
        n_pos = C.c_uint64(0)
        while True:
            calls = np.zeros(call_cap, dtype=SMEM_CALL)
            intv = np.zeros(intv_cap, dtype=SMEM_INTV)
            sa_off = np.zeros(intv_cap, dtype=np.uint64)
            sa_pos = np.zeros(sa_cap, dtype=np.uint64)
            rc = lib().bmh_seed_batch(self._h, _ptr(opt), C.c_int(int(max_occ)), n, C.cast(c_reads, C.c_void_p), _ptr(call_off), _ptr(calls),
                                      C.c_size_t(call_cap), _ptr(intv_off), _ptr(intv), C.c_size_t(intv_cap), _ptr(sa_off), _ptr(sa_pos),
                                      C.c_size_t(sa_cap), C.byref(n_pos))
            if rc != BMH_E_CIGAR_CAP:
                break
            call_cap, intv_cap, sa_cap = 2 * call_cap, 4 * intv_cap, 4 * sa_cap
        self._check(rc)
        out, offs = [], []
        for r in range(n):
            lo, hi = int(intv_off[r]), int(intv_off[r + 1])
            out.append((calls[call_off[r]:call_off[r + 1]].copy(), intv[lo:hi].copy()))
            offs.append(sa_off[lo:hi].copy())
        return out, offs, sa_pos[:n_pos.value].copy()

    def chain_batch(self, opt, l_pac, reads, calls, intvs, sa_off, sa_pos):
        """bmh_chain_batch: chaining on the GPU over per-read seeding tables (calls[r], intvs[r], sa_off[r] as seed_batch returns
        them, sa_pos the positions).  Returns per read a list of SEED arrays in chain order (what bmh_chain_reads gives)."""
        n = len(reads)
        o = np.ascontiguousarray(np.asarray(opt, dtype=CHAIN_OPT).reshape(()))
        keep = []
        c_reads = (_Read * max(n, 1))()
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
        call_off = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint32)
        intv_off = np.concatenate([[0], np.cumsum([len(v) for v in intvs])]).astype(np.uint64)
        fc = np.ascontiguousarray(np.concatenate(list(calls) + [np.zeros(1, SMEM_CALL)]), dtype=SMEM_CALL)
        fi = np.ascontiguousarray(np.concatenate(list(intvs) + [np.zeros(1, SMEM_INTV)]), dtype=SMEM_INTV)
        fo = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint64) for x in sa_off] + [np.zeros(1, np.uint64)]))
        pos = np.ascontiguousarray(np.concatenate([np.asarray(sa_pos, dtype=np.uint64), np.zeros(1, np.uint64)]))
        out = (_ChainV * max(n, 1))()
        self._check(lib().bmh_chain_batch(self._h, _ptr(o), C.c_int64(int(l_pac)), n, C.cast(c_reads, C.c_void_p), _ptr(call_off), _ptr(fc),
                                          _ptr(intv_off), _ptr(fi), _ptr(fo), _ptr(pos), C.c_uint64(len(pos) - 1), C.cast(out, C.c_void_p)))
        return _take_chains(out, n)

    def seed_chain_batch(self, smem_opt, chain_opt, l_pac, reads):
        """bmh_seed_chain_batch: seeding and chaining in one device round trip.  Returns per read a list of SEED arrays in chain
        order."""
        n = len(reads)
        o_in, so = np.asarray(smem_opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            so[k] = o_in[k]
        co = np.ascontiguousarray(np.asarray(chain_opt, dtype=CHAIN_OPT).reshape(()))
        keep = []
        c_reads = (_Read * max(n, 1))()
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
        out = (_ChainV * max(n, 1))()
        self._check(lib().bmh_seed_chain_batch(self._h, _ptr(so), _ptr(co), C.c_int64(int(l_pac)), n, C.cast(c_reads, C.c_void_p),
                                               C.cast(out, C.c_void_p)))
        return _take_chains(out, n)

    def chain_stats(self):
        """bmh_chain_stats of the last chaining call: dict of reads, chains_in / chains_out (around mem_chain_flt), seeds, equal_keys,
        kernel_ms."""
        st = _ChainStats()
        self._check(lib().bmh_chain_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in _ChainStats._fields_}

    def sa_batch(self, ks):
        """N x bwt_sa (reference bwt.c:85)."""
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        pos = np.zeros(len(ks), dtype=np.uint64)
        self._check(lib().bmh_sa_batch(self._h, _ptr(ks), len(ks), _ptr(pos)))
        return pos

    def matesw_batch(self, l_pac, pac, reads, regs, pes, opt, dedup):
        """Batched mate rescue (reference bwamem_pair.c:251-263 over mem_matesw :109-175) for len(reads)//2 pairs.
        reads: flat list of uint8 code arrays (2 per pair); regs: flat list of ALNREG arrays; pes: PESTAT[4];
        opt: MATESW_OPT record; dedup: C function pointer with the bmh_dedup_fn shape.
        Returns (regs after rescue, n per pair)."""
        n_pairs = len(reads) // 2
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        pes = np.ascontiguousarray(pes, dtype=PESTAT)
        opt = np.ascontiguousarray(opt, dtype=MATESW_OPT)
        keep = []
        c_reads = (_Read * len(reads))()
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
        c_regs = (_AlnregV * len(regs))()
        for k, r in enumerate(regs):
            r = np.ascontiguousarray(r, dtype=ALNREG)
            c_regs[k].n = c_regs[k].m = len(r)
            if len(r):
                c_regs[k].a = _libc.malloc(len(r) * ALNREG.itemsize)
                C.memmove(c_regs[k].a, r.ctypes.data, len(r) * ALNREG.itemsize)
        n_sw = np.zeros(max(n_pairs, 1), dtype=np.int32)
        rc = lib().bmh_matesw_batch(self._h, C.c_int64(l_pac), _ptr(pac), n_pairs, C.cast(c_reads, C.c_void_p),
                                    C.cast(c_regs, C.c_void_p), _ptr(pes), _ptr(opt), dedup, None, _ptr(n_sw))
        out = []
        for k in range(len(regs)):
            a = np.zeros(c_regs[k].n, dtype=ALNREG)
            if c_regs[k].n:
                C.memmove(a.ctypes.data, c_regs[k].a, c_regs[k].n * ALNREG.itemsize)
            if c_regs[k].a:
                _libc.free(c_regs[k].a)
            out.append(a)
        self._check(rc)
        return out, n_sw[:n_pairs].tolist()

    def matesw_device(self, l_pac, reads, regs, pes, opt, mask_level_redun):
        """bmh_matesw_device: the same driver as kernels, against the resident reference (set_pac); mem_sort_and_dedup runs on the
        device at mask_level_redun.  Arguments as matesw_batch's.  Returns (regs after rescue, n per pair).  A refused call raises
        BmhError with the vectors as the call left them in its `regs` attribute."""
        n_pairs = len(reads) // 2
        pes = np.ascontiguousarray(pes, dtype=PESTAT)
        opt = np.ascontiguousarray(opt, dtype=MATESW_OPT)
        keep = []
        c_reads = (_Read * max(len(reads), 1))()
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
        c_regs = (_AlnregV * max(len(regs), 1))()
        for k, r in enumerate(regs):
            r = np.ascontiguousarray(r, dtype=ALNREG)
            c_regs[k].n = c_regs[k].m = len(r)
            if len(r):
                c_regs[k].a = _libc.malloc(len(r) * ALNREG.itemsize)
                C.memmove(c_regs[k].a, r.ctypes.data, len(r) * ALNREG.itemsize)
        n_sw = np.zeros(max(n_pairs, 1), dtype=np.int32)
        rc = lib().bmh_matesw_device(self._h, C.c_int64(l_pac), n_pairs, C.cast(c_reads, C.c_void_p), C.cast(c_regs, C.c_void_p),
                                     _ptr(pes), _ptr(opt), C.c_float(mask_level_redun), _ptr(n_sw))
        out = []
        for k in range(len(regs)):
            a = np.zeros(c_regs[k].n, dtype=ALNREG)
            if c_regs[k].n:
                C.memmove(a.ctypes.data, c_regs[k].a, c_regs[k].n * ALNREG.itemsize)
            if c_regs[k].a:
                _libc.free(c_regs[k].a)
            out.append(a)
        try:
            self._check(rc)
        except BmhError as e:
            e.regs = out
            raise
        return out, n_sw[:n_pairs].tolist()

    def matesw_table_device(self, l_pac, reads, regs, pes, opt, mask_level_redun, roff=None):
        """bmh_matesw_table_device: matesw_device over a flat region table.  Arguments and result as matesw_device's: the vectors are
        flattened here (read k's regions at reg[roff[k]:roff[k + 1]]) and the output table is cut into vectors again.  roff: the
        offsets to pass instead of the vectors' own (for the argument checks).  A refused call raises BmhError with what it left of
        the outputs in `outputs`: (roff_out, the region pointer, n_sw), each as it was before the call if nothing was written."""
        n_pairs = len(reads) // 2
        pes = np.ascontiguousarray(pes, dtype=PESTAT)
        opt = np.ascontiguousarray(opt, dtype=MATESW_OPT)
        keep = []
        c_reads = (_Read * max(len(reads), 1))()
        for k, r in enumerate(reads):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            keep.append(r)
            c_reads[k].l_seq, c_reads[k].seq = len(r), r.ctypes.data
        vecs = [np.ascontiguousarray(r, dtype=ALNREG).reshape(-1) for r in regs]
        flat = np.concatenate([np.zeros(0, dtype=ALNREG)] + vecs)
        if roff is None:
            roff = np.concatenate([[0], np.cumsum([len(v) for v in vecs])])
        roff = np.ascontiguousarray(roff, dtype=np.uint64)
        roff_out = np.full(2 * n_pairs + 1, 0xdeadbeefdeadbeef, dtype=np.uint64)
        n_sw = np.full(max(n_pairs, 1), -77, dtype=np.int32)
        reg_out = C.c_void_p(None)
        rc = lib().bmh_matesw_table_device(self._h, C.c_int64(l_pac), n_pairs, C.cast(c_reads, C.c_void_p), _ptr(roff),
                                           _ptr(flat) if len(flat) else None, _ptr(pes), _ptr(opt), C.c_float(mask_level_redun), _ptr(roff_out),
                                           C.cast(C.byref(reg_out), C.c_void_p), _ptr(n_sw))
        try:
            self._check(rc)
        except BmhError as e:
            e.outputs = (roff_out, reg_out.value, n_sw[:n_pairs])
            raise
        total = int(roff_out[2 * n_pairs])
        table = np.zeros(total, dtype=ALNREG)
        if total:
            C.memmove(table.ctypes.data, reg_out.value, total * ALNREG.itemsize)
        _libc.free(reg_out)
        return [table[int(roff_out[k]):int(roff_out[k + 1])].copy() for k in range(2 * n_pairs)], n_sw[:n_pairs].tolist()

    def last_matesw_table_stats(self):
        """bmh_last_matesw_table_stats as a dict of MATESW_TABLE_STATS' fields: the last matesw_table_device call on this context."""
        st = np.zeros(1, dtype=MATESW_TABLE_STATS)
        self._check(lib().bmh_last_matesw_table_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in MATESW_TABLE_STATS.names}

    def extend_batch_device(self, d_pool, d_tasks, n, d_res, d_order=0):
        self._check(lib().bmh_extend_batch_device(self._h, C.c_void_p(d_pool), C.c_void_p(d_tasks), int(n),
                                                  C.c_void_p(d_res), C.c_void_p(d_order) if d_order else None))

    def global_batch_device(self, d_pool, d_tasks, n, d_res, d_cigar, d_order=0):
        self._check(lib().bmh_global_batch_device(self._h, C.c_void_p(d_pool), C.c_void_p(d_tasks), int(n),
                                                  C.c_void_p(d_res), C.c_void_p(d_cigar),
                                                  C.c_void_p(d_order) if d_order else None))

    # ---- L3 driver
    def chain2aln_batch(self, l_pac, pac, reads, chains):
        """reads: list of uint8 code arrays; chains: per read a list of SEED arrays.
        Returns per read an ALNREG array (what mem_chain2aln appends, reference bwamem.c:730-878)."""
        n = len(reads)
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        keep = []
        c_reads = (_Read * n)()
        c_chv = (_ChainV * n)()
        c_regs = (_AlnregV * n)()
        for r in range(n):
            seq = np.ascontiguousarray(reads[r], dtype=np.uint8)
            keep.append(seq)
            c_reads[r].l_seq, c_reads[r].seq = len(seq), seq.ctypes.data
            arr = (_Chain * max(len(chains[r]), 1))()
            for ci, seeds in enumerate(chains[r]):
                sd = np.ascontiguousarray(seeds, dtype=SEED)
                keep.append(sd)
                arr[ci].n = arr[ci].m = len(sd)
                arr[ci].pos = int(sd["rbeg"][0]) if len(sd) else 0
                arr[ci].seeds = sd.ctypes.data
            keep.append(arr)
            c_chv[r].n = c_chv[r].m = len(chains[r])
            c_chv[r].a = C.cast(arr, C.POINTER(_Chain))
        rc = lib().bmh_chain2aln_batch(self._h, int(l_pac), _ptr(pac), n, C.cast(c_reads, C.c_void_p),
                                       C.cast(c_chv, C.c_void_p), None, None, C.cast(c_regs, C.c_void_p))
        out = []
        for r in range(n):
            k = c_regs[r].n
            a = np.zeros(k, dtype=ALNREG)
            if k:
                C.memmove(a.ctypes.data, c_regs[r].a, k * ALNREG.itemsize)
            if c_regs[r].a:
                _libc.free(c_regs[r].a)
            out.append(a)
        self._check(rc)
        return out

    @staticmethod
    def _c_reads_chains(reads, chains):
        """(keep-alive list, bmh_read_t[n], bmh_chain_v[n] or None) of lists of code arrays / per read lists of SEED arrays."""
        n = len(reads)
        keep = []
        c_reads = (_Read * max(n, 1))()
        c_chv = (_ChainV * max(n, 1))() if chains is not None else None
        for r in range(n):
            seq = np.ascontiguousarray(reads[r], dtype=np.uint8)
            keep.append(seq)
            c_reads[r].l_seq, c_reads[r].seq = len(seq), seq.ctypes.data
            if chains is None:
                continue
            arr = (_Chain * max(len(chains[r]), 1))()
            for ci, seeds in enumerate(chains[r]):
                sd = np.ascontiguousarray(seeds, dtype=SEED)
                keep.append(sd)
                arr[ci].n = arr[ci].m = len(sd)
                arr[ci].pos = int(sd["rbeg"][0]) if len(sd) else 0
                arr[ci].seeds = sd.ctypes.data
            keep.append(arr)
            c_chv[r].n = c_chv[r].m = len(chains[r])
            c_chv[r].a = C.cast(arr, C.POINTER(_Chain))
        return keep, c_reads, c_chv

    def _take_regs(self, c_regs, n, rc):
        """bmh_alnreg_v[n] -> per read an ALNREG array; frees the C allocations, then raises on rc."""
        out = []
        for r in range(n):
            k = c_regs[r].n
            a = np.zeros(k, dtype=ALNREG)
            if k:
                C.memmove(a.ctypes.data, c_regs[r].a, k * ALNREG.itemsize)
            if c_regs[r].a:
                _libc.free(c_regs[r].a)
            out.append(a)
        self._check(rc)
        return out

    def chains2regs_batch(self, l_pac, pac, reads, chains, min_seed_len):
        """bmh_chains2regs_batch, the host driver: mem_chain2aln_short + mem_chain2aln per chain (min_seed_len >= 1).
        Returns per read an ALNREG array."""
        n = len(reads)
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        keep, c_reads, c_chv = self._c_reads_chains(reads, chains)
        c_regs = (_AlnregV * max(n, 1))()
        rc = lib().bmh_chains2regs_batch(self._h, int(l_pac), _ptr(pac), n, C.cast(c_reads, C.c_void_p), C.cast(c_chv, C.c_void_p),
                                         int(min_seed_len), C.cast(c_regs, C.c_void_p))
        return self._take_regs(c_regs, n, rc)

    def chains2regs_device(self, l_pac, reads, chains, min_seed_len=0, regs_in=None):
        """bmh_chains2regs_device: the same driver as kernels, against the resident reference (set_pac).  min_seed_len = 0: no
        short-chain pre-step.  regs_in (test hook): per read an ALNREG array the call finds in regs[r]; it must refuse them."""
        n = len(reads)
        keep, c_reads, c_chv = self._c_reads_chains(reads, chains)
        c_regs = (_AlnregV * max(n, 1))()
        for r, a in enumerate(regs_in or []):
            a = np.ascontiguousarray(a, dtype=ALNREG)
            if len(a):
                c_regs[r].n = c_regs[r].m = len(a)
                c_regs[r].a = _libc.malloc(len(a) * ALNREG.itemsize)
                C.memmove(c_regs[r].a, a.ctypes.data, len(a) * ALNREG.itemsize)
        rc = lib().bmh_chains2regs_device(self._h, int(l_pac), n, C.cast(c_reads, C.c_void_p), C.cast(c_chv, C.c_void_p),
                                          int(min_seed_len), C.cast(c_regs, C.c_void_p))
        return self._take_regs(c_regs, n, rc)

    def seed_chain_regs_batch(self, smem_opt, chain_opt, l_pac, reads, min_seed_len=0):
        """bmh_seed_chain_regs_batch: seeding, chaining and the chains-to-regions driver in one call; only regions come back.
        Returns per read an ALNREG array."""
        n = len(reads)
        o_in, so = np.asarray(smem_opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            so[k] = o_in[k]
        co = np.ascontiguousarray(np.asarray(chain_opt, dtype=CHAIN_OPT).reshape(()))
        keep, c_reads, _ = self._c_reads_chains(reads, None)
        c_regs = (_AlnregV * max(n, 1))()
        rc = lib().bmh_seed_chain_regs_batch(self._h, _ptr(so), _ptr(co), C.c_int64(int(l_pac)), n, C.cast(c_reads, C.c_void_p),
                                             int(min_seed_len), C.cast(c_regs, C.c_void_p))
        return self._take_regs(c_regs, n, rc)

    def sort_dedup_batch(self, vectors, mask_level_redun):
        """bmh_sort_dedup_batch: mem_sort_and_dedup for every vector of a batch in one device call.
        vectors: per read an ALNREG array (left as it is).  Returns per read the ALNREG array of the survivors, in order."""
        n = len(vectors)
        bufs = [np.array(v, dtype=ALNREG, copy=True).reshape(-1) for v in vectors]
        c_regs = (_AlnregV * max(n, 1))()
        for r, a in enumerate(bufs):
            c_regs[r].n = c_regs[r].m = len(a)
            c_regs[r].a = a.ctypes.data if len(a) else None
        self._check(lib().bmh_sort_dedup_batch(self._h, n, C.cast(c_regs, C.c_void_p), float(mask_level_redun)))
        return [a[:c_regs[r].n].copy() for r, a in enumerate(bufs)]

    def set_regs_dedup(self, on=True, mask_level_redun=0.95):
        """bmh_ctx_set_regs_dedup: while on, chains2regs_device and seed_chain_regs_batch return what mem_sort_and_dedup
        leaves of their regions (sorted and filtered on the device, before the download)."""
        self._check(lib().bmh_ctx_set_regs_dedup(self._h, 1 if on else 0, float(mask_level_redun)))

    def last_dedup_stats(self):
        """(regions in, regions kept, kernel ms or -1) of the last call that ran the de-duplication kernel; -1 each before it."""
        a, b, ms = C.c_int64(0), C.c_int64(0), C.c_float(0)
        self._check(lib().bmh_last_dedup_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)))
        return a.value, b.value, ms.value

    def pestat_device(self, opt, l_pac, vectors):
        """bmh_pestat_device: mem_pestat's pair walk for a caller's vectors in one device call.  Arguments and result as
        pestat_candidates()."""
        return _pestat_words(self, opt, l_pac, vectors)

    def set_regs_drop_exact(self, on=True):
        """bmh_ctx_set_regs_drop_exact: while on (with set_regs_dedup on), chains2regs_device and seed_chain_regs_batch apply
        mem_test_and_remove_exact on the device, behind the de-duplication."""
        self._check(lib().bmh_ctx_set_regs_drop_exact(self._h, 1 if on else 0))

    def set_pestat_collect(self, on=True, opt=None):
        """bmh_ctx_set_pestat_collect: while on (with set_regs_dedup on), the two calls also compute mem_pestat's word per pair of
        reads (2p, 2p+1) under opt (SAM_OPT, copied); last_pestat_candidates() hands them out."""
        o = np.array(opt, dtype=SAM_OPT).reshape(1) if opt is not None else None
        self._check(lib().bmh_ctx_set_pestat_collect(self._h, 1 if on else 0, _ptr(o) if o is not None else None))

    def last_pestat_candidates(self, n_pairs):
        """(words, kernel ms or -1) of the last successful collecting call, which had n_pairs pairs."""
        w, ms = np.zeros(max(int(n_pairs), 0), dtype=np.uint32), C.c_float(0)
        self._check(lib().bmh_last_pestat_candidates(self._h, _ptr(w) if len(w) else None, int(n_pairs), C.byref(ms)))
        return w, ms.value

    def last_drop_exact_stats(self):
        """Regions drop-exact removed in the last successful call that ran with it on; -1 before the first."""
        a = C.c_int64(0)
        self._check(lib().bmh_last_drop_exact_stats(self._h, C.byref(a)))
        return a.value

    def decide_device(self, opt, l_pac, pes, id0, vectors, roff=None, inplace=False):
        """bmh_decide_device: pass A of phase 2 as a kernel.  Arguments and result as decide_batch()."""
        return _decide(self, opt, l_pac, pes, id0, vectors, roff, inplace)

    def set_decide_device(self, on=True):
        """bmh_ctx_set_decide_device: while on, bmh_sam_batch takes its pass A from bmh_decide_device."""
        self._check(lib().bmh_ctx_set_decide_device(self._h, 1 if on else 0))

    def last_decide_stats(self):
        """(units decided on the device, 1 if the call answered BMH_E_RANGE else 0, kernel ms or -1) of the last bmh_decide_device call."""
        a, b, ms = C.c_int64(0), C.c_int64(0), C.c_float(0)
        self._check(lib().bmh_last_decide_stats(self._h, C.byref(a), C.byref(b), C.byref(ms)))
        return a.value, b.value, ms.value

    def set_refidx(self, refidx):
        """bmh_ctx_set_refidx: (offset, len) of every reference sequence resident on the device; None drops it."""
        self._check(lib().bmh_ctx_set_refidx(self._h, C.byref(refidx) if refidx is not None else None))

    def set_wanted_device(self, on=True):
        """bmh_ctx_set_wanted_device: while on, bmh_sam_batch takes its pass B from bmh_wanted_cigar_device."""
        self._check(lib().bmh_ctx_set_wanted_device(self._h, 1 if on else 0))

    def last_wanted_stats(self):
        """(wanted regions, regions fixed, regions redone on the host, planning-kernel ms or -1) of the last bmh_wanted_cigar_device call."""
        a, b, c, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        self._check(lib().bmh_last_wanted_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)))
        return a.value, b.value, c.value, ms.value

    def wanted_cigar_batch(self, refidx, pac, w, reads, vectors, want, device=False, out=None):
        """bmh_wanted_cigar_batch (device=True: bmh_wanted_cigar_device): pass B of phase 2.  reads: uint8 code arrays; vectors: per read an
        ALNREG array; want: per read the indices of its wanted regions.  Returns (WANTED_RES records, CIGAR pool, MD bytes); out: the three
        arrays to write into (a test's sentinels)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        n = len(reads)
        keep = []
        c_reads = (_Read * max(n, 1))()
        c_regs = (_AlnregV * max(n, 1))()
        for r, (seq, v) in enumerate(zip(reads, vectors)):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            v = np.ascontiguousarray(v, dtype=ALNREG).reshape(-1)
            keep += [seq, v]
            c_reads[r].l_seq, c_reads[r].seq = len(seq), seq.ctypes.data
            c_regs[r].n = c_regs[r].m = len(v)
            c_regs[r].a = v.ctypes.data if len(v) else None
        roff = np.concatenate([[0], np.cumsum([len(v) for v in vectors])]).astype(np.int64)
        n_want = np.array([len(x) for x in want], dtype=np.int32).reshape(-1)
        want_k = np.full(int(roff[-1]) + 1, -1, dtype=np.int32)
        span = 0
        for i, ks in enumerate(want):
            want_k[int(roff[i]):int(roff[i]) + len(ks)] = ks
            for k in ks:
                if 0 <= k < len(vectors[i]):
                    a = vectors[i][k]
                    span += max(int(a["qe"]) - int(a["qb"]), 0) + max(int(a["re"]) - int(a["rb"]), 0)
        n_w = int(n_want.sum())
        if out is None:
            out = (np.zeros(n_w, dtype=WANTED_RES), np.zeros(span + 2 * n_w + 8, dtype=np.uint32), np.zeros(3 * span + 16 * n_w + 16, dtype=np.uint8))
        res, cig, md = out
        fn = lib().bmh_wanted_cigar_device if device else lib().bmh_wanted_cigar_batch
        self._check(fn(self._h, C.byref(refidx), _ptr(pac), int(w), n, C.cast(c_reads, C.c_void_p), C.cast(c_regs, C.c_void_p), _ptr(roff),
                       _ptr(n_want), _ptr(want_k), _ptr(res), _ptr(cig), C.c_size_t(len(cig)), _ptr(md), C.c_size_t(len(md))))
        return res, cig, md

    def phase2_device(self, opt, refidx, pac, pes, id0, reads, vectors, inplace=False, out=None, results_cap=None):
        """bmh_phase2_device: pass A and pass B of phase 2 as one device session.  opt: SAM_OPT (w = opt.w); reads: uint8 code arrays;
        vectors: per read an ALNREG array (left as it is, or with inplace=True worked on where it lies).  Returns decide_batch()'s dict
        with res (WANTED_RES records, n_wanted of them), cig, md and n_wanted added.  out: arrays to write into by name (pd, reg_mapq,
        n_want, want_k, res, cig, md: a test's sentinels); results_cap: the capacity to state for res, else its length."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        n = len(reads)
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        bufs = list(vectors) if inplace else [np.array(v, dtype=ALNREG, copy=True).reshape(-1) for v in vectors]
        keep = []
        c_reads = (_Read * max(n, 1))()
        c_regs = (_AlnregV * max(n, 1))()
        for r, (seq, a) in enumerate(zip(reads, bufs)):
            assert a.dtype == ALNREG and a.flags.c_contiguous
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            keep.append(seq)
            c_reads[r].l_seq, c_reads[r].seq = len(seq), seq.ctypes.data
            c_regs[r].n = c_regs[r].m = len(a)
            c_regs[r].a = a.ctypes.data if len(a) else None
        roff = np.concatenate([[0], np.cumsum([len(a) for a in bufs])]).astype(np.int64)
        total = int(roff[-1])
        span = sum(max(int(x["qe"]) - int(x["qb"]), 0) + max(int(x["re"]) - int(x["rb"]), 0) for a in bufs for x in a)
        pe = bool(int(o["flag"][0]) & MEM_F_PE)
        out = dict(out or {})
        got = {"pd": np.zeros(n // 2 if pe else 0, dtype=PAIRDEC), "reg_mapq": np.full(total, -1, dtype=np.int32),
               "want_k": np.full(total, -1, dtype=np.int32), "n_want": np.full(n, -1, dtype=np.int32), "res": np.zeros(total, dtype=WANTED_RES),
               "cig": np.zeros(span + 2 * total + 8, dtype=np.uint32), "md": np.zeros(3 * span + 16 * total + 16, dtype=np.uint8)}
        got.update(out)
        n_wanted = C.c_int64(-1)
        pes_p = _ptr(np.ascontiguousarray(pes, dtype=PESTAT)) if pes is not None else None
        rc = lib().bmh_phase2_device(self._h, _ptr(o), C.byref(refidx), _ptr(pac), pes_p, C.c_int64(int(id0)), n, C.cast(c_reads, C.c_void_p),
                                     C.cast(c_regs, C.c_void_p), _ptr(roff), _ptr(got["pd"]) if pe else None, _ptr(got["reg_mapq"]), _ptr(got["n_want"]),
                                     _ptr(got["want_k"]), _ptr(got["res"]), C.c_int64(len(got["res"]) if results_cap is None else int(results_cap)),
                                     C.cast(C.byref(n_wanted), C.c_void_p), _ptr(got["cig"]), C.c_size_t(len(got["cig"])), _ptr(got["md"]),
                                     C.c_size_t(len(got["md"])))
        self._check(rc)
        got["regs"], got["n_wanted"] = bufs, n_wanted.value
        got["res"] = got["res"][:n_wanted.value]
        got["want"] = [got["want_k"][int(roff[i]):int(roff[i]) + int(got["n_want"][i])].copy() for i in range(n)]
        return got

    def set_phase2_device(self, on=True):
        """bmh_ctx_set_phase2_device: while on, bmh_sam_batch takes pass A and pass B from bmh_phase2_device."""
        self._check(lib().bmh_ctx_set_phase2_device(self._h, 1 if on else 0))

    def last_phase2_stats(self):
        """bmh_last_phase2_stats as a dict of PHASE2_STATS' fields: the last fused call on this context."""
        st = np.zeros(1, dtype=PHASE2_STATS)
        self._check(lib().bmh_last_phase2_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in PHASE2_STATS.names}

    def set_refnames(self, refidx):
        """bmh_ctx_set_refnames: the name of every reference sequence resident on the device; None drops it."""
        self._check(lib().bmh_ctx_set_refnames(self._h, C.byref(refidx) if refidx is not None else None))

    def set_samtext_device(self, on=True):
        """bmh_ctx_set_samtext_device: while on, bmh_sam_batch takes its pass C from bmh_sam_text_device."""
        self._check(lib().bmh_ctx_set_samtext_device(self._h, 1 if on else 0))

    def last_samtext_stats(self):
        """bmh_last_samtext_stats as a dict of SAMTEXT_STATS' fields: the last bmh_sam_text_device call on this context."""
        st = np.zeros(1, dtype=SAMTEXT_STATS)
        self._check(lib().bmh_last_samtext_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in SAMTEXT_STATS.names if k != "rsv"}

    def phase2_text_device(self, opt, refidx, pac, pes, id0, seqs, vectors, rg_id=b"", out=None):
        """bmh_phase2_text_device: passes A, B and C of phase 2 as one device session, only the text comes down.  opt: SAM_OPT; seqs: per
        read (name, comment or None, uint8 base codes, qualities or None); vectors: per read an ALNREG array, read where it lies and
        left as it is (an array of another dtype or layout is copied first).  Returns (text, text_off): the pool's bytes and n + 1
        offsets.  out: {"text": a C.c_void_p, "text_off": an int64 array} to write into (a test's sentinels)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8) if pac is not None else None
        n = len(seqs)
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        keep = []
        c_seqs = (_Seq * max(n, 1))()
        c_regs = (_AlnregV * max(n, 1))()
        for r, ((name, comment, seq, qual), v) in enumerate(zip(seqs, vectors)):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            v = np.ascontiguousarray(v, dtype=ALNREG).reshape(-1)
            keep += [seq, v]
            c_seqs[r] = _Seq(len(seq), name, comment, seq.ctypes.data if len(seq) else None, qual, None)
            c_regs[r].n = c_regs[r].m = len(v)
            c_regs[r].a = v.ctypes.data if len(v) else None
        out = out or {}
        text = out.get("text", C.c_void_p(None))
        text_off = out.get("text_off", np.zeros(n + 1, dtype=np.int64))
        pes_p = _ptr(np.ascontiguousarray(pes, dtype=PESTAT)) if pes is not None else None
        self._check(lib().bmh_phase2_text_device(self._h, _ptr(o), C.byref(refidx) if refidx is not None else None, _ptr(pac), pes_p, C.c_int64(int(id0)), n,
                                                 C.cast(c_seqs, C.c_void_p), C.cast(c_regs, C.c_void_p), rg_id, C.cast(C.byref(text), C.c_void_p),
                                                 _ptr(text_off)))
        data = C.string_at(text.value, int(text_off[n]))
        _libc.free(text)
        return data, text_off

    def set_phase2_text_device(self, on=True):
        """bmh_ctx_set_phase2_text_device: while on, bmh_sam_batch takes all three passes from bmh_phase2_text_device."""
        self._check(lib().bmh_ctx_set_phase2_text_device(self._h, 1 if on else 0))

    def last_phase2_text_stats(self):
        """bmh_last_phase2_text_stats as a dict of PHASE2_TEXT_STATS' fields: the last such call on this context."""
        st = np.zeros(1, dtype=PHASE2_TEXT_STATS)
        self._check(lib().bmh_last_phase2_text_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in PHASE2_TEXT_STATS.names if k != "rsv"}

    def reads_sam_device(self, smem_opt, chain_opt, min_seed_len, opt, refidx, pac, id0, seqs, rg_id=b"", out=None):
        """bmh_reads_sam_device: single-end reads to SAM text as one device session; the regions never leave the device.  smem_opt,
        chain_opt, min_seed_len as seed_chain_regs_batch's, opt (SAM_OPT), refidx, pac, id0, seqs, rg_id and out as
        phase2_text_device's.  Returns (text, text_off)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8) if pac is not None else None
        n = len(seqs)
        o_in, so = np.asarray(smem_opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            so[k] = o_in[k]
        co = np.ascontiguousarray(np.asarray(chain_opt, dtype=CHAIN_OPT).reshape(()))
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        keep = []
        c_seqs = (_Seq * max(n, 1))()
        for r, (name, comment, seq, qual) in enumerate(seqs):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            keep.append(seq)
            c_seqs[r] = _Seq(len(seq), name, comment, seq.ctypes.data if len(seq) else None, qual, None)
        out = out or {}
        text = out.get("text", C.c_void_p(None))
        text_off = out.get("text_off", np.zeros(n + 1, dtype=np.int64))
        self._check(lib().bmh_reads_sam_device(self._h, _ptr(so), _ptr(co), int(min_seed_len), _ptr(o), C.byref(refidx) if refidx is not None else None,
                                               _ptr(pac), C.c_int64(int(id0)), n, C.cast(c_seqs, C.c_void_p), rg_id, C.cast(C.byref(text), C.c_void_p),
                                               _ptr(text_off)))
        data = C.string_at(text.value, int(text_off[n]))
        _libc.free(text)
        return data, text_off

    def last_reads_sam_stats(self):
        """bmh_last_reads_sam_stats as a dict of READS_SAM_STATS' fields: the last reads_sam_device call on this context."""
        st = np.zeros(1, dtype=READS_SAM_STATS)
        self._check(lib().bmh_last_reads_sam_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in READS_SAM_STATS.names if k != "rsv"}

    def pairs_sam_device(self, smem_opt, chain_opt, min_seed_len, matesw_opt, opt, refidx, pac, pes, id0, seqs, rg_id=b"", out=None):
        """bmh_pairs_sam_device: paired-end reads to SAM text as one device session; the regions never leave the device.  Reads 2p and
        2p + 1 are mates.  matesw_opt: MATESW_OPT; pes: the caller's PESTAT[4], or None for the table of exactly these reads; the rest as
        reads_sam_device's.  Returns (text, text_off, pes): pes is the table that was used.  out may also hold "pes", a PESTAT[4] array
        to write into."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8) if pac is not None else None
        n = len(seqs)
        o_in, so = np.asarray(smem_opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            so[k] = o_in[k]
        co = np.ascontiguousarray(np.asarray(chain_opt, dtype=CHAIN_OPT).reshape(()))
        mo = np.ascontiguousarray(matesw_opt, dtype=MATESW_OPT)
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        keep = []
        c_seqs = (_Seq * max(n, 1))()
        for r, (name, comment, seq, qual) in enumerate(seqs):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            keep.append(seq)
            c_seqs[r] = _Seq(len(seq), name, comment, seq.ctypes.data if len(seq) else None, qual, None)
        out = out or {}
        text = out.get("text", C.c_void_p(None))
        text_off = out.get("text_off", np.zeros(n + 1, dtype=np.int64))
        pes_out = out.get("pes", np.zeros(4, dtype=PESTAT))
        pes_p = _ptr(np.ascontiguousarray(pes, dtype=PESTAT)) if pes is not None else None
        self._check(lib().bmh_pairs_sam_device(self._h, _ptr(so), _ptr(co), int(min_seed_len), _ptr(mo), _ptr(o),
                                               C.byref(refidx) if refidx is not None else None, _ptr(pac), pes_p, _ptr(pes_out), C.c_int64(int(id0)), n,
                                               C.cast(c_seqs, C.c_void_p), rg_id, C.cast(C.byref(text), C.c_void_p), _ptr(text_off)))
        data = C.string_at(text.value, int(text_off[n]))
        _libc.free(text)
        return data, text_off, pes_out

    @staticmethod
    def _c_seqs(seqs):
        """(name, comment, seq, qual) tuples as a bmh_seq_t array, and what keeps its pointers alive"""
        keep = []
        c_seqs = (_Seq * max(len(seqs), 1))()
        for r, (name, comment, seq, qual) in enumerate(seqs):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            keep.append(seq)
            c_seqs[r] = _Seq(len(seq), name, comment, seq.ctypes.data if len(seq) else None, qual, None)
        return c_seqs, keep

    def pairs_sam_begin(self, smem_opt, chain_opt, min_seed_len, opt, refidx, seqs, collect=True):
        """bmh_pairs_sam_begin: phase 1 of the paired-end session, its table and bases parked in a device block of their own.  Returns
        (parked, cand): a ParkedPairs for pairs_sam_finish on any context of the same device, and the n / 2 insert-size words (None
        with collect=False)."""
        n = len(seqs)
        o_in, so = np.asarray(smem_opt), np.zeros((), dtype=SMEM_OPT)
        for k in o_in.dtype.names:
            so[k] = o_in[k]
        co = np.ascontiguousarray(np.asarray(chain_opt, dtype=CHAIN_OPT).reshape(()))
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        c_seqs, keep = self._c_seqs(seqs)
        cand = np.zeros(n // 2, dtype=np.uint32) if collect else None
        h = C.c_void_p(None)
        self._check(lib().bmh_pairs_sam_begin(self._h, _ptr(so), _ptr(co), int(min_seed_len), _ptr(o), C.byref(refidx) if refidx is not None else None,
                                              n, C.cast(c_seqs, C.c_void_p), _ptr(cand), C.cast(C.byref(h), C.c_void_p)))
        return ParkedPairs(h.value), cand

    def pairs_sam_finish(self, parked, matesw_opt, opt, refidx, pac, pes, id0, seqs, rg_id=b""):
        """bmh_pairs_sam_finish: mate rescue, the plan and phase 2 over what pairs_sam_begin parked, under the table pes (PESTAT[4]).
        Returns (text, text_off).  A call refused before anything ran leaves `parked` valid; past that it is consumed."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8) if pac is not None else None
        n = len(seqs)
        mo = np.ascontiguousarray(matesw_opt, dtype=MATESW_OPT)
        o = np.array(opt, dtype=SAM_OPT).reshape(1)
        c_seqs, keep = self._c_seqs(seqs)
        text = C.c_void_p(None)
        text_off = np.zeros(n + 1, dtype=np.int64)
        pes = np.ascontiguousarray(pes, dtype=PESTAT)
        rc = lib().bmh_pairs_sam_finish(self._h, parked._h, _ptr(mo), _ptr(o), C.byref(refidx) if refidx is not None else None, _ptr(pac), _ptr(pes),
                                        C.c_int64(int(id0)), n, C.cast(c_seqs, C.c_void_p), rg_id, C.cast(C.byref(text), C.c_void_p), _ptr(text_off))
        if lib().bmh_pairs_finish_consumed(self._h):
            parked._h = None
        self._check(rc)
        data = C.string_at(text.value, int(text_off[n]))
        _libc.free(text)
        return data, text_off

    def last_pairs_sam_stats(self):
        """bmh_last_pairs_sam_stats as a dict of PAIRS_SAM_STATS' fields: the last pairs_sam_device or pairs_sam_finish call on this context."""
        st = np.zeros(1, dtype=PAIRS_SAM_STATS)
        self._check(lib().bmh_last_pairs_sam_stats(self._h, _ptr(st)))
        return {k: st[0][k].item() for k in PAIRS_SAM_STATS.names if k != "rsv"}

    def sam_text_batch(self, *args, device=True, **kw):
        """sam_text_batch() on this context: bmh_sam_text_device (device=False: the host call, which needs no context)."""
        return sam_text_batch(*args, ctx=self if device else None, **kw)

    def reg2cigar_batch(self, l_pac, pac, reads, reqs):
        """Batched mem_reg2aln band/retry loop over bwa_gen_cigar2 (reference bwamem.c:1187-1201, bwa.c:89-172).
        reads: list of uint8 code arrays; reqs: CIGAR_REQ array.  Returns (results, cigar_pool, md_bytes)."""
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        reqs = np.ascontiguousarray(reqs, dtype=CIGAR_REQ)
        keep = []
        c_reads = (_Read * max(len(reads), 1))()
        for r, seq in enumerate(reads):
            seq = np.ascontiguousarray(seq, dtype=np.uint8)
            keep.append(seq)
            c_reads[r].l_seq, c_reads[r].seq = len(seq), seq.ctypes.data
        span = (reqs["qe"] - reqs["qb"]).astype(np.int64) + (reqs["re"] - reqs["rb"]).astype(np.int64)
        span = np.maximum(span, 0)
        cw, mb = int(span.sum() + 2 * len(reqs) + 8), int(3 * span.sum() + 16 * len(reqs) + 16)
        res = np.zeros(len(reqs), dtype=CIGAR_RES)
        cig = np.zeros(cw, dtype=np.uint32)
        md = np.zeros(mb, dtype=np.uint8)
        self._check(lib().bmh_reg2cigar_batch(self._h, int(l_pac), _ptr(pac), C.cast(c_reads, C.c_void_p), len(reqs),
                                              _ptr(reqs), _ptr(res), _ptr(cig), cw, _ptr(md), mb))
        return res, cig, md

    def driver_stats(self):
        st = _DriverStats()
        self._check(lib().bmh_driver_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _DriverStats._fields_}


def _decide(ctx, opt, l_pac, pes, id0, vectors, roff, inplace):
    n = len(vectors)
    o = np.array(opt, dtype=SAM_OPT).reshape(1)
    bufs = list(vectors) if inplace else [np.array(v, dtype=ALNREG, copy=True).reshape(-1) for v in vectors]
    c_regs = (_AlnregV * max(n, 1))()
    for r, a in enumerate(bufs):
        assert a.dtype == ALNREG and a.flags.c_contiguous
        c_regs[r].n = c_regs[r].m = len(a)
        c_regs[r].a = a.ctypes.data if len(a) else None
    if roff is None:
        roff = np.concatenate([[0], np.cumsum([len(a) for a in bufs])])
    roff = np.ascontiguousarray(roff, dtype=np.int64)
    total = int(sum(len(a) for a in bufs))
    pe = bool(int(o["flag"][0]) & MEM_F_PE)
    pd = np.zeros(n // 2 if pe else 0, dtype=PAIRDEC)
    reg_mapq, want_k, n_want = np.full(total, -1, dtype=np.int32), np.full(total, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    pes_p = _ptr(np.ascontiguousarray(pes, dtype=PESTAT)) if pes is not None else None
    args = (_ptr(o), C.c_int64(int(l_pac)), pes_p, C.c_int64(int(id0)), n, C.cast(c_regs, C.c_void_p), _ptr(roff), _ptr(pd) if pe else None,
            _ptr(reg_mapq), _ptr(n_want), _ptr(want_k))
    rc = lib().bmh_decide_batch(*args) if ctx is None else lib().bmh_decide_device(ctx._h, *args)
    if rc:
        raise BmhError(rc, lib().bmh_strerror(rc).decode() if ctx is None else lib().bmh_last_error(ctx._h).decode())
    want = [want_k[int(roff[i]):int(roff[i]) + int(n_want[i])].copy() for i in range(n)]
    return {"regs": bufs, "pd": pd, "reg_mapq": reg_mapq, "n_want": n_want, "want_k": want_k, "want": want}


def decide_batch(opt, l_pac, pes, id0, vectors, roff=None, inplace=False):
    """bmh_decide_batch: pass A of phase 2 on the host -- primary marking, pairing (opt.flag has MEM_F_PE: vectors 2p, 2p+1 are
    mates, pes = PESTAT[4]), mapQ and the list of regions that get printed.  vectors: per read an ALNREG array (left as it is, or
    with inplace=True worked on where it lies).
    Returns a dict: regs (per read the vector as pass A leaves it), pd (PAIRDEC per pair), reg_mapq, n_want, want_k (flat, at the
    regions' offsets; entries past n_want stay -1) and want (per read the printed regions' indices)."""
    return _decide(None, opt, l_pac, pes, id0, vectors, roff, inplace)


def _pestat_words(ctx, opt, l_pac, vectors):
    n = len(vectors)
    o = np.array(opt, dtype=SAM_OPT).reshape(1)
    bufs = [np.ascontiguousarray(v, dtype=ALNREG).reshape(-1) for v in vectors]
    c_regs = (_AlnregV * max(n, 1))()
    for r, a in enumerate(bufs):
        c_regs[r].n = c_regs[r].m = len(a)
        c_regs[r].a = a.ctypes.data if len(a) else None
    cand = np.zeros(n // 2, dtype=np.uint32)
    cp = _ptr(cand) if len(cand) else None
    if ctx is None:
        rc = lib().bmh_pestat_candidates(_ptr(o), int(l_pac), n, C.cast(c_regs, C.c_void_p), cp)
        if rc:
            raise BmhError(rc, lib().bmh_strerror(rc).decode())
    else:
        ctx._check(lib().bmh_pestat_device(ctx._h, _ptr(o), int(l_pac), n, C.cast(c_regs, C.c_void_p), cp))
    return cand


def pestat_candidates(opt, l_pac, vectors):
    """bmh_pestat_candidates: mem_pestat's pair walk on the host.  opt: SAM_OPT; vectors: per read an ALNREG array, reads 2p and
    2p+1 being mates (an odd count ignores the last).  Returns len(vectors) // 2 words: 0 = no candidate, else
    orientation << 30 | insert size."""
    return _pestat_words(None, opt, l_pac, vectors)


def pestat_from_candidates(opt, cand, verbose=-1):
    """bmh_pestat_from_candidates: mem_pestat's statistics from such words.  Returns PESTAT[4]."""
    o = np.array(opt, dtype=SAM_OPT).reshape(1)
    cand = np.ascontiguousarray(cand, dtype=np.uint32).reshape(-1)
    pes = np.zeros(4, dtype=PESTAT)
    rc = lib().bmh_pestat_from_candidates(_ptr(o), len(cand), _ptr(cand) if len(cand) else None, _ptr(pes), int(verbose))
    if rc:
        raise BmhError(rc, lib().bmh_strerror(rc).decode())
    return pes


def sam_text_batch(opt, refidx, pes, seqs, vectors, dec, res, cig, md, rg_id=b"", ctx=None, out=None):
    """bmh_sam_text_batch (with ctx: bmh_sam_text_device on it): pass C of phase 2, the SAM text of a slice.  seqs: per read (name,
    comment or None, uint8 base codes, qualities or None); vectors: per read its ALNREG array as pass A left it; dec: pass A's outputs
    by name (pd, reg_mapq, n_want, want_k: decide_batch()'s dict); res, cig, md: pass B's records and pools.  Returns (text, text_off):
    the pool's bytes and n + 1 offsets.  out: {"text": a C.c_void_p, "text_off": an int64 array} to write into (a test's sentinels)."""
    n = len(seqs)
    o = np.array(opt, dtype=SAM_OPT).reshape(1)
    pe = bool(int(o["flag"][0]) & MEM_F_PE)
    keep = []
    c_seqs = (_Seq * max(n, 1))()
    c_regs = (_AlnregV * max(n, 1))()
    for r, ((name, comment, seq, qual), v) in enumerate(zip(seqs, vectors)):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        v = np.ascontiguousarray(v, dtype=ALNREG).reshape(-1)
        keep += [seq, v]
        c_seqs[r] = _Seq(len(seq), name, comment, seq.ctypes.data if len(seq) else None, qual, None)
        c_regs[r].n = c_regs[r].m = len(v)
        c_regs[r].a = v.ctypes.data if len(v) else None
    roff = np.concatenate([[0], np.cumsum([len(v) for v in vectors])]).astype(np.int64)
    arr = {k: (np.ascontiguousarray(dec[k]) if dec.get(k) is not None else None) for k in ("pd", "reg_mapq", "n_want", "want_k")}
    res = np.ascontiguousarray(res, dtype=WANTED_RES) if res is not None else None
    cig = np.ascontiguousarray(cig, dtype=np.uint32) if cig is not None else None
    md = np.ascontiguousarray(md, dtype=np.uint8) if md is not None else None
    out = out or {}
    text = out.get("text", C.c_void_p(None))
    text_off = out.get("text_off", np.zeros(n + 1, dtype=np.int64))
    pes_p = _ptr(np.ascontiguousarray(pes, dtype=PESTAT)) if pes is not None else None
    args = (_ptr(o), C.byref(refidx) if refidx is not None else None, pes_p, n, C.cast(c_seqs, C.c_void_p), C.cast(c_regs, C.c_void_p), _ptr(roff),
            _ptr(arr["pd"]) if pe else None, _ptr(arr["reg_mapq"]), _ptr(arr["n_want"]), _ptr(arr["want_k"]), _ptr(res), _ptr(cig), _ptr(md), rg_id,
            C.cast(C.byref(text), C.c_void_p), _ptr(text_off))
    rc = lib().bmh_sam_text_batch(*args) if ctx is None else lib().bmh_sam_text_device(ctx._h, *args)
    if rc:
        raise BmhError(rc, lib().bmh_strerror(rc).decode() if ctx is None else lib().bmh_last_error(ctx._h).decode())
    data = C.string_at(text.value, int(text_off[n]))
    _libc.free(text)
    return data, text_off


def extend_batch_sharded(ctxs, pool, tasks):
    """Static contiguous shard of one host batch over several contexts (one per GPU)."""
    return _sharded("bmh_extend_batch_sharded", ctxs, pool, tasks, EXT_TASK, EXT_RES)


def _sharded(fn, ctxs, pool, tasks, tdtype, rdtype, *more):
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    tasks = np.ascontiguousarray(tasks, dtype=tdtype)
    res = np.zeros(len(tasks), dtype=rdtype)
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    rc = getattr(lib(), fn)(arr, len(ctxs), _ptr(pool), C.c_size_t(pool.nbytes), _ptr(tasks), C.c_int64(len(tasks)), _ptr(res), *more)
    if rc:
        raise BmhError(rc, lib().bmh_strerror(rc).decode())
    return res


def seedext_batch_sharded(ctxs, pool, tasks):
    """Fused per-seed records, one contiguous slice per context (bmh_seedext_batch_sharded)."""
    return _sharded("bmh_seedext_batch_sharded", ctxs, pool, tasks, SEED_TASK, SEED_RES)


def sw_batch_sharded(ctxs, pool, tasks):
    """ksw_align2 tasks, one contiguous slice per context (bmh_sw_batch_sharded)."""
    return _sharded("bmh_sw_batch_sharded", ctxs, pool, tasks, SW_TASK, SW_RES)


def global_batch_sharded(ctxs, pool, tasks, cigar_words):
    """ksw_global2 + traceback, one contiguous slice per context (bmh_global_batch_sharded) -> (results, CIGAR pool)."""
    cig = np.zeros(max(int(cigar_words), 1), dtype=np.uint32)
    res = _sharded("bmh_global_batch_sharded", ctxs, pool, tasks, GLB_TASK, GLB_RES, _ptr(cig), C.c_size_t(int(cigar_words)))
    return res, cig


def declared_symbols():
    """Every function name declared in include/bwamem_hip.h (for the symbol-export test)."""
    import re
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bmh_[a-z0-9_]+)\s*\(", txt)))
