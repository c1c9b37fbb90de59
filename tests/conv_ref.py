"""float64 NumPy references for the convolution tests, and pure-Python statements of the launch selection of
csrc/conv_direct.hip (which kernel template a shape reaches, on how many workgroups).

The references state nn/functional.py:254-281 (im2col + GEMM, col2im) and, for the fused chain, functional.py:31-32 /
284-339 with the reference's tie semantics (tensor.py:808-815).  They walk the batch in blocks of BLOCK images: the
im2col matrix of a 1027-image batch never exists at once, only the outputs do."""
import numpy as np

BLOCK = 64


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _cols(xb, k, s, p):
    """im2col of a block: rows (n, oy, ox), columns (c, kh, kw); also the padded block's shape."""
    xp = np.pad(xb, [(0, 0), (0, 0), (p, p), (p, p)])
    n, C, PH, PW = xp.shape
    oh, ow = (PH - k) // s + 1, (PW - k) // s + 1
    s0, s1, s2, s3 = xp.strides
    col = np.lib.stride_tricks.as_strided(xp, (n, C, k, k, oh, ow), (s0, s1, s2, s3, s2 * s, s3 * s))
    return col.transpose(0, 4, 5, 1, 2, 3).reshape(n * oh * ow, C * k * k), xp.shape


def _col2im(dcol, shape, k, s, p, oh, ow):
    """dcol (n, oh, ow, C, k, k) scattered back into the padded image, tap by tap (what np.add.at on the strided
    window view computes, without its per-element cost); returns the unpadded interior."""
    n, C, PH, PW = shape
    dxp = np.zeros(shape)
    d = dcol.transpose(0, 3, 4, 5, 1, 2)
    for kh in range(k):
        for kw in range(k):
            dxp[:, :, kh:kh + s * (oh - 1) + 1:s, kw:kw + s * (ow - 1) + 1:s] += d[:, :, kh, kw]
    return dxp[:, :, p:PH - p, p:PW - p]


def conv_ref(x, w, b, g, s, p, block=BLOCK):
    """y, dx, dw, db of y = conv2d(x, w, stride s, pad p) + b under the upstream gradient g (b may be None)."""
    x, w, g = (a.astype(np.float64) for a in (x, w, g))
    N, C, H, W = x.shape
    O, _, k, _ = w.shape
    oh, ow = out_hw(H, W, k, s, p)
    w2 = w.reshape(O, -1)
    y, dx = np.empty((N, O, oh, ow)), np.empty((N, C, H, W))
    dw, db = np.zeros((O, C * k * k)), np.zeros(O)
    for n0 in range(0, N, block):
        sl = slice(n0, min(N, n0 + block))
        a, pshape = _cols(x[sl], k, s, p)
        n = pshape[0]
        yb = a @ w2.T
        if b is not None:
            yb = yb + b.astype(np.float64)
        y[sl] = yb.reshape(n, oh, ow, O).transpose(0, 3, 1, 2)
        g2 = g[sl].transpose(0, 2, 3, 1).reshape(n * oh * ow, O)
        dw += g2.T @ a
        db += g2.sum(0)
        dx[sl] = _col2im((g2 @ w2).reshape(n, oh, ow, C, k, k), pshape, k, s, p, oh, ow)
    return y, dx, dw.reshape(w.shape), db


def conv_relu_pool_ref(x, w, b, gp, s=1, p=1, block=BLOCK):
    """pooled = max_pool2d(relu(conv2d(x, w) + b), 2, 2) and the gradients of sum(pooled * gp) w.r.t. x, w, b.
    Ties: EVERY window position whose relu equals the window maximum receives the pooled gradient, and relu passes it
    where relu(y) == y, i.e. also at y == 0 (maximum(0., y): tensor.py:808-815)."""
    x, w, gp = (a.astype(np.float64) for a in (x, w, gp))
    N, C, H, W = x.shape
    O, _, k, _ = w.shape
    oh, ow = out_hw(H, W, k, s, p)
    assert oh % 2 == 0 and ow % 2 == 0
    w2 = w.reshape(O, -1)
    pooled, dx = np.empty((N, O, oh // 2, ow // 2)), np.empty((N, C, H, W))
    dw, db = np.zeros((O, C * k * k)), np.zeros(O)
    for n0 in range(0, N, block):
        sl = slice(n0, min(N, n0 + block))
        a, pshape = _cols(x[sl], k, s, p)
        n = pshape[0]
        yb = a @ w2.T
        if b is not None:
            yb = yb + b.astype(np.float64)
        y = yb.reshape(n, oh, ow, O).transpose(0, 3, 1, 2)
        r = np.maximum(0.0, y)
        win = r.reshape(n, O, oh // 2, 2, ow // 2, 2)
        pb = win.max((3, 5))
        pooled[sl] = pb
        dr = ((win == pb[:, :, :, None, :, None]) * gp[sl][:, :, :, None, :, None]).reshape(n, O, oh, ow)
        dy = (r == y) * dr
        g2 = dy.transpose(0, 2, 3, 1).reshape(n * oh * ow, O)
        dw += g2.T @ a
        db += g2.sum(0)
        dx[sl] = _col2im((g2 @ w2).reshape(n, oh, ow, C, k, k), pshape, k, s, p, oh, ow)
    return pooled, dx, dw.reshape(w.shape), db


def integer_inputs(rng, N, C, H, W, O, k, g_shape):
    """x in {-2..2}, w / bias / upstream gradient in {-1, 0, 1}: every product and partial sum of the three
    directions is an integer below 2^24 for the shapes of these tests, so fp32 is exact in ANY summation order."""
    return (rng.integers(-2, 3, (N, C, H, W)).astype(np.float32), rng.integers(-1, 2, (O, C, k, k)).astype(np.float32),
            rng.integers(-1, 2, (O,)).astype(np.float32), rng.integers(-1, 2, g_shape).astype(np.float32))


def normal_inputs(rng, N, C, H, W, O, k, g_shape):
    return (rng.standard_normal((N, C, H, W), dtype=np.float32), rng.standard_normal((O, C, k, k), dtype=np.float32),
            rng.standard_normal((O,), dtype=np.float32), rng.standard_normal(g_shape, dtype=np.float32))


# ---- csrc/conv_direct.hip: launch_direct's selection ------------------------------------------------------------
_MAX_LDS = 150 * 1024


def forward_variant(C, H, W, O, k, s, p, N):
    """(OT, CH, KS, NV, grid) of conv_direct_kernel<OT, CH, KS, NV> for the forward of this shape (launch_direct):
    output tiles x position chunks per wave, the unrolled tap count (0: the generic loop), float4 registers per
    thread that prefetch the next image (0: staged straight into LDS), workgroups."""
    oh, ow = out_hw(H, W, k, s, p)
    cp, opad = (C + 1) // 2 * 2, (O + 31) // 32 * 32
    lds = 4 * (k * k * cp * opad + cp * (H + 2 * p) * (W + 2 * p) + opad) + 64
    assert opad <= 64 and lds <= _MAX_LDS, "outside the direct kernel"
    per_cu = 1 if _MAX_LDS // lds < 1 else (160 * 1024) // lds
    grid = min(256 * min(per_cu, 4), N)
    chunks = (oh * ow + 31) // 32
    in_elems = C * H * W
    nv = (in_elems // 4 + 255) // 256 if (W % 4 == 0 and in_elems <= 16 * 1024) else 0
    if opad == 64:
        ot, ch = (2, 2) if chunks >= 8 else (2, 1)
    else:
        ot, ch = (1, 4) if chunks >= 16 else (1, 2) if chunks >= 8 else (1, 1)
    ks = 3 if k == 3 else 5 if (k == 5 and ot * ch <= 2) else 1 if k == 1 else 0
    nvt = 0 if (nv == 0 or ks != 3) else 4 if nv <= 4 else 8 if nv <= 8 else 16
    return ot, ch, ks, nvt, grid


def dgrad_variant(C, H, W, O, k, s, p, N):
    """The data gradient is the same kernel on (dy, flipped w): input O x OH x OW, output C channels, pad k-1-p."""
    assert s == 1 and k - 1 - p >= 0
    oh, ow = out_hw(H, W, k, s, p)
    return forward_variant(O, oh, ow, C, k, 1, k - 1 - p, N)


def wgrad_variant(C, H, W, O, k, s, p, N, pooled_source=False):
    """launch_wgrad's selection.  ("lean", KT, OTN, NVD, MB, halved, grid, per_block) for conv_wgrad_lean_kernel<KT,
    OTN, 8, NVD>, or ("regular", WT, PS, prefetch, MB, False, grid, per_block) for conv_wgrad_kernel<WT, PS, ...>:
    `grid` workgroups each take `per_block` consecutive images (the last one what is left)."""
    oh, ow = out_hw(H, W, k, s, p)
    PH, PW, M = H + 2 * p, W + 2 * p, oh * ow
    opad, k1 = (O + 31) // 32 * 32, C * k * k + 1
    kcols = (k1 + 31) // 32 * 32
    MB = 512 if (4 * C * PH * PW + 4 * (O + 1) * (M | 1) > 78 * 1024 and M > 512) else M
    T = (opad // 32) * (kcols // 32)
    lds = max(4 * (C * PH * PW + (O + 1) * (MB | 1)) + 64, 4 * 4 * 3 * 16 * 64)
    assert T <= 16 and lds <= _MAX_LDS, "outside the direct kernel"
    blocks = min(256 * min((160 * 1024) // lds, 2), N)
    per_block = (N + blocks - 1) // blocks
    grid = (N + per_block - 1) // per_block
    KT, OTN = kcols // 32, opad // 32

    def lean_lds(mb):
        return max(4 * ((C + 2) * PH * PW + (O + 1) * ((mb + 2) | 1)) + 64, 4 * (4 // OTN - 1) * OTN * KT * 16 * 64)

    def prefetch(mb):
        return W % 4 == 0 and M % 4 == 0 and mb % 4 == 0 and C * H * W <= 8 * 1024 and O * min(mb, M) <= 16 * 1024

    mb, halved = MB, False
    if (lean_lds(mb) > 80 * 1024 or (kcols >= 128 and O * (mb // 4) > 8 * 256)) and mb % 8 == 0 and mb > 128:
        mb, halved = mb // 2, True
    need = (O * (mb // 4) + 255) // 256
    lean = (1 <= KT <= 6 and OTN in (1, 2) and mb % 4 == 0 and k1 <= 6 * 32 and prefetch(mb) and lean_lds(mb) <= 80 * 1024
            and M % mb == 0 and mb % 32 == 0 and mb % (2 * ow) == 0 and need <= (8 if KT >= 4 else 16)
            and (not pooled_source or (ow % 4 == 0 and oh % 2 == 0 and M % 32 == 0)) and ow % 2 == 0)
    if lean:
        return "lean", KT, OTN, 8 if need <= 8 else 16, mb, halved, grid, per_block
    ps = 1 if T < 4 else 0
    return "regular", T if ps else (T + 3) // 4, ps, prefetch(MB), MB, False, grid, per_block


def quad_grids(C, H, W, O, N):
    """csrc/conv_quad.hip on LeNet's two layers: (forward, data-gradient, weight-gradient) workgroups and the images
    one forward / data-gradient work item holds (a 32-lane tile is one row of 32 positions or one row of two images)."""
    assert (C, H, W, O) in ((3, 32, 32, 20), (20, 16, 16, 50))
    ipt = 32 // W
    wgs = 2 if O <= 32 else 1                        # (a second workgroup per CU where there is one channel tile)
    groups = (N + ipt - 1) // ipt
    return min(groups, 256 * wgs), min((N + 3) // 4, 256), min(N, 256), ipt
