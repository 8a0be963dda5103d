"""Decoders of the 2-bit reference array for tests that address targets by doubled coordinate (BMH_F_TPAC, the region record)."""
import numpy as np


def fwd(pac, f0, n):
    """n forward-strand bases from f0 on, decoded from the 2-bit array"""
    idx = np.arange(f0, f0 + n, dtype=np.int64)
    return ((pac[idx >> 2] >> ((~idx & 3) << 1).astype(np.uint8)) & 3).astype(np.uint8)


def window(pac, l_pac, pos, n):
    """n bases of the doubled coordinate from pos on (bntseq.c:355-376), decoded from the 2-bit array"""
    if pos >= l_pac:  # reverse strand: complement of the forward strand read backwards
        f0 = 2 * l_pac - pos - n
        return (3 - fwd(pac, f0, n))[::-1]
    return fwd(pac, pos, n)
