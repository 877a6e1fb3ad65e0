"""numpy helpers for the tests: bf16 bit conversion and the packed fragment-tile format
(markushgrapher_amd/csrc/mg_device.h), restated independently of the HIP code."""
import numpy as np


def bf16_bits(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16).reshape(x.shape)


def bf16_to_f32(bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32).reshape(bits.shape)


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x))


def pack_tiles(x, rows_pad=None):
    """X[R][K] fp32 -> packed bf16 bits [R/32][K/16][2][32][8] flattened."""
    R, K = x.shape
    Rp = rows_pad if rows_pad is not None else (R + 31) // 32 * 32
    xb = np.zeros((Rp, K), np.uint16)
    xb[:R] = bf16_bits(x)
    t = xb.reshape(Rp // 32, 32, K // 16, 2, 8)          # [rt][row][kt][half][8]
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)


def unpack_tiles(bits, R, K):
    """inverse of pack_tiles -> fp32 [R][K] (R multiple of 32 of the stored rows)."""
    Rp = bits.size // K
    t = np.asarray(bits, np.uint16).reshape(Rp // 32, K // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4)
    return bf16_to_f32(np.ascontiguousarray(t).reshape(Rp, K))[:R]


def unpack_heads_rows(bits, B, H, S_cap):
    """HF_PK_ROWS [B][H][S_cap/32][4][2][32][8] -> fp32 [B][H][S_cap][64]"""
    t = np.asarray(bits, np.uint16).reshape(B, H, S_cap // 32, 4, 2, 32, 8).transpose(0, 1, 2, 5, 3, 4, 6)
    return bf16_to_f32(np.ascontiguousarray(t).reshape(B, H, S_cap, 64))


def unpack_heads_t(bits, B, H, S_cap):
    """HF_PK_T [B][H][2][S_cap/16][2][32][8] (rows = dim, k = token) -> fp32 [B][H][S_cap][64]"""
    t = np.asarray(bits, np.uint16).reshape(B, H, 2, S_cap // 16, 2, 32, 8)   # [b][h][dt][kt][half][dim32][8tok]
    t = t.transpose(0, 1, 3, 4, 6, 2, 5)                                       # [b][h][kt][half][8][dt][dim32]
    return bf16_to_f32(np.ascontiguousarray(t).reshape(B, H, S_cap, 64))


def unpack_tile_bits(bits, K):
    """packed bf16 bits -> the stored bit patterns as uint16 [rows stored][K] (padding rows included)."""
    Rp = bits.size // K
    t = np.asarray(bits, np.uint16).reshape(Rp // 32, K // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4)
    return np.ascontiguousarray(t).reshape(Rp, K)


def tile_f32(h, pad_value=0.0):
    """fp32 H[M][N] -> the tiled residual-stream layout [M/32][N/4][32 rows][4 features] flattened (ht_off in mg_device.h: element
    (m, n) at ((m // 32) * (N // 4) + n // 4) * 128 + (m % 32) * 4 + n % 4); rows M .. M rounded up to 32 hold pad_value."""
    M, N = h.shape
    Mp = (M + 31) // 32 * 32
    hp = np.full((Mp, N), pad_value, np.float32)
    hp[:M] = h
    return np.ascontiguousarray(hp.reshape(Mp // 32, 32, N // 4, 4).transpose(0, 2, 1, 3)).reshape(-1)


def untile_f32(t, N):
    """inverse of tile_f32 -> fp32 [rows stored][N] (padding rows included)."""
    Mp = t.size // N
    return np.ascontiguousarray(np.asarray(t, np.float32).reshape(Mp // 32, N // 4, 32, 4).transpose(0, 2, 1, 3)).reshape(Mp, N)


def pack_tile_bits(bits2d):
    """uint16 bit patterns [Rp][K] (Rp a multiple of 32) -> the packed tile format, flattened: inverse of unpack_tile_bits."""
    Rp, K = bits2d.shape
    t = np.asarray(bits2d, np.uint16).reshape(Rp // 32, 32, K // 16, 2, 8)
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)


def window_bits(x, ld, col0, fill_bits, rows_pad=None):
    """A packed buffer of `ld` columns whose columns [col0, col0 + x.shape[1]) hold bf16(x) in rows [0, x.shape[0]) and whose every other
    element (other columns, padding rows) holds the bit pattern `fill_bits`: an activation WINDOW of a wider buffer (x_kts / x_k0 of the
    decode-step kernels: k-tile window [col0 / 16, (col0 + K) / 16)) or the target of a column-window output (x2_ld / x2_col0)."""
    R, K = x.shape
    Rp = rows_pad if rows_pad is not None else (R + 31) // 32 * 32
    b = np.full((Rp, ld), fill_bits, np.uint16)
    b[:R, col0:col0 + K] = bf16_bits(x)
    return pack_tile_bits(b)
