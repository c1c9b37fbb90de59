"""Float64 statements of what pdn_gemm_f32, pdn_linear_relu_fwd_f32 and pdn_linear_dx_masked_f32 compute (include/pdn_hip.h),
for tests/test_gemm_variants.py.  Plain NumPy on the logical operands: no strides, no tiles, no splits."""
import numpy as np

F32, F64 = np.float32, np.float64


def gemm(a, b, alpha=1.0, bias=None, residual=None, beta=0.0, c0=None):
    """alpha * a @ b + bias + residual + beta * c0 over any leading batch dimensions (c0 is not read when beta is 0)."""
    r = float(alpha) * np.matmul(np.asarray(a, F64), np.asarray(b, F64))
    if bias is not None:
        r = r + np.asarray(bias, F64)
    if residual is not None:
        r = r + np.asarray(residual, F64)
    if beta != 0.0:
        r = r + float(beta) * np.asarray(c0, F64)
    return r


def colsum(b, prior, accumulate):
    """Column sums of the (K x N) operand B, added to what the buffer held when `accumulate`."""
    s = np.asarray(b, F64).sum(0)
    return s + np.asarray(prior, F64) if accumulate else s


def pack_bits(keep):
    """(rows x cols) booleans -> (rows x cols / 32) uint32 words, bit c of word [row][col / 32] = column 32 (col / 32) + c."""
    keep = np.ascontiguousarray(keep, bool)
    rows, cols = keep.shape
    assert cols % 32 == 0
    return np.packbits(keep, axis=1, bitorder="little").view(np.uint32).reshape(rows, cols // 32)


def unpack_bits(words, cols):
    words = np.ascontiguousarray(words, np.uint32)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], cols // 8), axis=1, bitorder="little").astype(bool)


def linear_relu(x, w, bias=None):
    """z = x w + bias; returns (z, max(0, z), z >= 0)."""
    z = np.matmul(np.asarray(x, F64), np.asarray(w, F64))
    if bias is not None:
        z = z + np.asarray(bias, F64)
    return z, np.maximum(0.0, z), z >= 0.0


def dx_masked(g, w, keep, existing=None):
    """dx = keep o (g w^T + existing), w (fin x fout); and its column sums over bands of 32 rows (the last may be short)."""
    r = np.matmul(np.asarray(g, F64), np.asarray(w, F64).T)
    if existing is not None:
        r = r + np.asarray(existing, F64)
    r = np.where(keep, r, 0.0)
    rows, fin = r.shape
    nb = (rows + 31) // 32
    pad = np.zeros((nb * 32, fin), F64)
    pad[:rows] = r
    return r, pad.reshape(nb, 32, fin).sum(1)


def round_bf16(x):
    """float32 -> nearest-even bfloat16, returned as float32."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F32).reshape(np.shape(x))


def rel_err(got, want):
    """Max-norm relative error (tests/test_kernels_gpu.py: rel_err)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)) if want.size else 0.0
