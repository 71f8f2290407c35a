"""CPU restatement of wavelet dithering (WaveletDitherStrategy.dither, dithering_lib.py:846-941), written from its
semantics -- test infrastructure only.

  * pywt.dwt2 / idwt2 (1.x, mode 'symmetric', float32): dec_terms lists, per output of the downsampling convolution, the
    (tap, input index) pairs in the order pywt's four C loops add them (left overhang, interior, filter longer than the
    line, right overhang); the synthesis adds sum_even / sum_odd of the valid upsampling convolution into a zeroed row,
    the approximation's first.  Taps: pywt's float32 filters (wavelet.json "taps", read off pywt with impulses).
  * _quant_subband with numpy 1.x scalar semantics: (sub - mn) / float32(float64(scale) + 1e-9); Q < 65536 in float32,
    larger Q in float64 (a Python int of uint32 size no longer casts to float32 under value-based casting); a constant
    subband draws nothing
  * the k=2 pick with scipy's KDTree and the float64 thresholds that follow every subband draw
"""
import numpy as np

WAVELETS = ("haar", "db1", "db2", "db4", "sym2", "sym4", "coif1", "bior1.3", "bior2.2")
f32 = np.float32


def dec_terms(N, F):
    """per output o (convolution index i = 2 o + 1): the (tap, input index) pairs in pywt's order of addition"""
    out = []

    def left_mirror(t, j):
        while j < F:
            k = 0
            while k < N and j < F:
                t.append((j, k))
                j += 1
                k += 1
            k = 0
            while k < N and j < F:
                t.append((j, N - 1 - k))
                j += 1
                k += 1

    for i in range(1, N + F - 1, 2):
        if i < F and i < N:
            t = [(j, i - j) for j in range(i + 1)]
            left_mirror(t, i + 1)
        elif i < N:
            t = [(j, i - j) for j in range(F)]
        else:
            t, j = [], 0
            while i - j >= N:
                k = 0
                while k < N and i - j >= N:
                    t.append((i - N - j, N - 1 - k))
                    j += 1
                    k += 1
                k = 0
                while k < N and i - j >= N:
                    t.append((i - N - j, k))
                    j += 1
                    k += 1
            if i < F:
                t += [(m, i - m) for m in range(j, i + 1)]
                left_mirror(t, i + 1)
            else:
                t += [(m, i - m) for m in range(j, F)]
        out.append(t)
    return out


def dwt_lines(x, lo, hi):
    """x: float32 [L, N] -> (approximation, detail) float32 [L, (N + F - 1) // 2]"""
    L, N = x.shape
    terms = dec_terms(N, len(lo))
    a = np.empty((L, len(terms)), f32)
    d = np.empty((L, len(terms)), f32)
    for o, t in enumerate(terms):
        sa = np.zeros(L, f32)
        sd = np.zeros(L, f32)
        for m, k in t:
            sa = sa + lo[m] * x[:, k]
            sd = sd + hi[m] * x[:, k]
        a[:, o], d[:, o] = sa, sd
    return a, d


def idwt_lines(a, d, lo, hi):
    """valid upsampling convolution of a with lo plus that of d with hi: float32 [L, 2 n - F + 2]"""
    L, n = a.shape
    F = len(lo)
    out = np.zeros((L, 2 * n - F + 2), f32)
    for oi, i in enumerate(range(F // 2 - 1, n)):
        for src, flt in ((a, lo), (d, hi)):
            se = np.zeros(L, f32)
            so = np.zeros(L, f32)
            for j in range(F // 2):
                se = se + flt[2 * j] * src[:, i - j]
                so = so + flt[2 * j + 1] * src[:, i - j]
            out[:, 2 * oi] += se
            out[:, 2 * oi + 1] += so
    return out


def taps_of(fixture_taps, wavelet):
    return {k: np.asarray(v, f32) for k, v in fixture_taps[wavelet].items()}


def dwt2(x, T):
    """float32 [h, w] -> cA, cH, cV, cD (dwtn's aa, da, ad, dd)"""
    lo, hi = T["dec_lo"], T["dec_hi"]
    a0, d0 = dwt_lines(np.ascontiguousarray(x.T), lo, hi)
    a0, d0 = np.ascontiguousarray(a0.T), np.ascontiguousarray(d0.T)
    aa, ad = dwt_lines(a0, lo, hi)
    da, dd = dwt_lines(d0, lo, hi)
    return aa, da, ad, dd


def idwt2(cA, cH, cV, cD, T):
    lo, hi = T["rec_lo"], T["rec_hi"]
    a = idwt_lines(cA, cV, lo, hi)   # axis 1 first: (aa, ad) and (da, dd)
    d = idwt_lines(cH, cD, lo, hi)
    return idwt_lines(np.ascontiguousarray(a.T), np.ascontiguousarray(d.T), lo, hi).T


def quant_subband(sub, Q, u):
    """_quant_subband with the next uniforms u (float64, at least sub.size); returns (result, values drawn)"""
    mn, mx = sub.min(), sub.max()
    if mx == mn:
        return sub.astype(f32), 0
    noise = u[:sub.size].reshape(sub.shape).astype(f32)
    scale = f32(mx - mn)
    den = f32(np.float64(scale) + 1e-9)
    norm = ((sub - mn) / den).astype(f32)
    if Q < 65536:
        q = np.floor(norm * f32(Q) + noise)
        q = np.minimum(np.maximum(q, f32(0)), f32(Q - 1))
        out = (q / f32(Q - 1 + 1e-9)) * scale + mn
    else:
        q = np.floor(norm.astype(np.float64) * float(Q) + noise.astype(np.float64))
        q = np.minimum(np.maximum(q, 0.0), float(Q - 1))
        out = (q / (Q - 1 + 1e-9)) * np.float64(scale) + np.float64(mn)
    return out.astype(f32), sub.size


def uniforms(seed, h, w, F):
    n0, n1 = (h + F - 1) // 2, (w + F - 1) // 2
    return np.random.RandomState(seed).random_sample(12 * n0 * n1 + h * w)


def reconstruct(img_f32, T, Q, u):
    """float32 [h, w, 3] -> (float32 [h, w, 3] clipped reconstruction, uniforms consumed, subbands per channel)"""
    h, w, _ = img_f32.shape
    res = np.zeros((h, w, 3), f32)
    pos, subs = 0, []
    for ch in range(3):
        bands = dwt2(np.ascontiguousarray(img_f32[:, :, ch]), T)
        subs.append(bands)
        qb = []
        for b in bands:
            r, n = quant_subband(b, Q, u[pos:])
            qb.append(r)
            pos += n
        rec = idwt2(*qb, T)[:h, :w]
        res[:, :, ch] = np.minimum(np.maximum(rec, f32(0)), f32(255))
    return res, pos, subs


def pick(points, pal_f32, thr):
    """the k=2 selection (dithering_lib.py:912-925): palette indices"""
    from scipy.spatial import KDTree
    dist, idx = KDTree(pal_f32).query(points.reshape(-1, 3), k=2)
    dsq = dist ** 2
    tot = dsq[:, 0] + dsq[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        factor = np.where(tot == 0, 0.0, dsq[:, 0] / tot)
    return np.where(factor <= thr, idx[:, 0], idx[:, 1])


def dither_indices(img_f32, pal_f32, taps, wavelet="haar", subband_quant=8, seed=42):
    """WaveletDitherStrategy(wavelet, subband_quant, seed).dither as palette indices [h * w] (img_f32: [h, w, 3])"""
    T = taps_of(taps, wavelet)
    h, w, _ = img_f32.shape
    u = uniforms(seed, h, w, len(T["dec_lo"]))
    rec, pos, _ = reconstruct(img_f32, T, subband_quant, u)
    return pick(rec, pal_f32, u[pos:pos + h * w])


def apply(arr_u8, palette, use_gamma, taps, **params):
    """ImageDitherer(..., DitherMode.WAVELET, palette, use_gamma, params).apply_dithering as a uint8 [h, w, 3] array"""
    from oracle import oracle as orc
    pal_f32, out_colors, lut_in = orc.prepare_palette(palette, use_gamma)
    src = arr_u8 if lut_in is None else np.asarray(lut_in)[arr_u8]
    h, w, _ = arr_u8.shape
    idx = dither_indices(src.astype(f32), pal_f32, taps, **params)
    return out_colors[idx].reshape(h, w, 3)


def make_input(spec):
    """the fixture inputs (tests/golden/make_golden_wavelet.py: make_input)"""
    from oracle import oracle as orc
    kind = spec[0]
    if kind == "rnd":
        return orc.rnd(spec[1], spec[2], spec[3])
    if kind == "grad":
        return orc.grad(spec[1], spec[2])
    if kind == "imgl":
        return orc.imgl(spec[1], spec[2], spec[3])
    if kind == "flat":
        return np.ascontiguousarray(np.broadcast_to(np.array(spec[3], np.uint8), (spec[1], spec[2], 3)))
    if kind == "flatch":
        a = orc.imgl(spec[1], spec[2], spec[3]).copy()
        a[..., spec[4]] = spec[5]
        return a
    if kind == "two":
        y, x = np.mgrid[0:spec[1], 0:spec[2]]
        v = np.where(((x // 8) + (y // 8)) % 2 == 0, spec[3], spec[4]).astype(np.uint8)
        return np.ascontiguousarray(np.stack([v, v, v], -1))
    raise ValueError(spec)
