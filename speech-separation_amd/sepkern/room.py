"""Image-method room impulse responses (Allen & Berkley 1979) with Peterson's (1986) low-pass images: the rooms that array
dynamic mixing simulates.  A rigid shoebox L = (Lx, Ly, Lz) metres with one reflection coefficient per wall, beta = (x0, x1, y0,
y1, z0, z1), each in [0, 1]; a source and a microphone strictly inside it; c = 343 m/s.

For every parity p in {0, 1}^3 and every m in Z^3 the image of the source lies, seen from the microphone, at

    R_a = (1 - 2 p_a) src_a + 2 m_a L_a - mic_a,    d = |R|,    tau = d rate / c  samples,
    A   = scale * prod_a beta_a0^|m_a - p_a| beta_a1^|m_a| / (4 pi d),    0^0 = 1,

and adds a Hann-windowed sinc of 64 taps around tau:  taps n = floor(tau) - 31 + j, j = 0 .. 63, t = n - tau in (-32, 32],

    h[n] += A * 0.5 (1 + cos(2 pi t / 64)) * sinc(t),    only 0 <= n < ntaps kept.

An image counts if A != 0 and floor(tau) - 31 <= ntaps - 1; per axis |m_a| <= ceil((ntaps + 32) c / (rate 2 L_a)) + 1 holds them
all (points inside the box have no image nearer than the direct path, and image 2 m_a L_a lies at least (2 |m_a| - 1) L_a away).

Below: `ism_rir`, that definition in fp64; `ism_rir_f32`, the numpy float32 restatement of what sk_room_rirs (csrc/room.hip)
computes -- the documentation of its arithmetic and the yardstick of the GPU test's tolerance, as reverb.convolve_partitioned_f32
is for csrc/fir.hip --; `tap_unit`, the unit that tolerance is counted in; Eyring's absorption, the random room geometry of a
training mixture and the array file.  numpy only: the loader's worker processes import this, not torch.
"""
import numpy as np

C_SOUND = 343.0              # m/s
WIDTH = 64                   # taps per image
HALF = 31                    # an image's first tap is floor(tau) - HALF
MAX_TAPS = 8192              # reverb.MAX_TAPS: what sk_fir_convolve takes
MAX_MICS = 8
MIN_DIRECT = 0.01            # metres: a source nearer to a microphone than this is refused
WAVES = 16                   # sk_room_rirs: private accumulators per workgroup (see ism_rir_f32)
FOUR_PI = 4.0 * np.pi
_BLOCK = 1 << 15             # images per vectorised block below


def _check(L, beta, src, mic, rate, ntaps):
    L, beta, src, mic = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (L, beta, src, mic))
    if L.shape != (3,) or beta.shape != (6,) or src.shape != (3,) or mic.shape != (3,):
        raise ValueError("room: L, src and mic have 3 numbers each, beta 6 (x0, x1, y0, y1, z0, z1)")
    if not np.all(L > 0.0) or not np.all((beta >= 0.0) & (beta <= 1.0)):
        raise ValueError("room: positive room dimensions and reflection coefficients in [0, 1] expected")
    if not (np.all((src > 0.0) & (src < L)) and np.all((mic > 0.0) & (mic < L))):
        raise ValueError("room: source and microphone lie strictly inside the box")
    if float(np.sqrt(np.sum((src - mic) ** 2))) < MIN_DIRECT:
        raise ValueError("room: source and microphone are less than %g m apart" % MIN_DIRECT)
    if not float(rate) >= 1.0 or not 1 <= int(ntaps) <= MAX_TAPS:
        raise ValueError("room: rate >= 1 and 1 <= ntaps <= %d expected" % MAX_TAPS)
    return L, beta, src, mic, float(rate), int(ntaps)


def image_range(L, rate, ntaps):
    """Per axis the M_a with |m_a| <= M_a for every image that counts: ceil((ntaps + 32) c / (rate 2 L_a)) + 1, formed in fp64 in
    exactly this order (the kernel's host side forms the same numbers)."""
    return [int(np.ceil((float(ntaps) + 32.0) * C_SOUND / (float(rate) * 2.0 * float(La)))) + 1 for La in L]


def _ipow(b, e):
    """b^e for integer arrays e >= 0 by binary exponentiation, multiplications in the order the kernel does them; 0^0 = 1."""
    e = np.array(e, dtype=np.int64)
    r = np.ones(e.shape, dtype=np.float64)
    b = np.full(e.shape, float(b), dtype=np.float64)
    while np.any(e > 0):
        odd = (e & 1) == 1
        r = np.where(odd, r * b, r)
        e = e >> 1
        b = b * b
    return r


def _images(L, beta, src, mic, rate, ntaps, scale, lo, hi, M, same_exponent=False):
    """Images lo .. hi - 1 of the kernel's enumeration (index i: parity p = i & 7 with p_x its bit 0; i >> 3 runs over m with m_z
    fastest, every m_a from -M_a up): (k = floor(tau), tau - k, A, counts?, [m_x, m_y, m_z]) -- all fp64 but k and m."""
    i = np.arange(lo, hi, dtype=np.int64)
    p = [(i >> a) & 1 for a in range(3)]
    q = i >> 3
    nz, ny = 2 * M[2] + 1, 2 * M[1] + 1
    m = [q // (nz * ny) - M[0], (q // nz) % ny - M[1], q % nz - M[2]]
    g = np.ones(i.shape, dtype=np.float64)
    d2 = None
    for a in range(3):
        R = (1.0 - 2.0 * p[a]) * src[a] + 2.0 * m[a] * L[a] - mic[a]
        d2 = R * R if d2 is None else d2 + R * R
        e1 = np.abs(m[a])
        e0 = e1 if same_exponent else np.abs(m[a] - p[a])
        g = (g * _ipow(beta[2 * a], e0)) * _ipow(beta[2 * a + 1], e1)
    d = np.sqrt(d2)
    tau = d * (rate / C_SOUND)
    k = np.floor(tau)
    A = (scale * g) / (FOUR_PI * d)
    counts = (A != 0.0) & (k - HALF <= ntaps - 1)
    return k.astype(np.int64), tau - k, A, counts, m


def count_images(L, beta, src, mic, rate, ntaps):
    """How many images count for this RIR."""
    L, beta, src, mic, rate, ntaps = _check(L, beta, src, mic, rate, ntaps)
    M = image_range(L, rate, ntaps)
    total = 8 * (2 * M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1)
    return sum(int(_images(L, beta, src, mic, rate, ntaps, 1.0, lo, min(lo + _BLOCK, total), M)[3].sum()) for lo in range(0, total, _BLOCK))


def ism_rir(L, beta, src, mic, rate, ntaps, scale=1.0, want_unit=False):
    """The definition in fp64 -> h (ntaps,) float64.  want_unit: -> (h, u) with u = tap_unit's array (one enumeration for both)."""
    L, beta, src, mic, rate, ntaps = _check(L, beta, src, mic, rate, ntaps)
    M = image_range(L, rate, ntaps)
    total = 8 * (2 * M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1)
    h = np.zeros(ntaps + 2 * WIDTH, dtype=np.float64)          # taps -64 .. ntaps + 63: clipped at the end
    cover = np.zeros(ntaps + 2 * WIDTH + 1, dtype=np.float64)
    j = np.arange(WIDTH, dtype=np.int64)
    for lo in range(0, total, _BLOCK):
        k, f, A, counts, _ = _images(L, beta, src, mic, rate, ntaps, float(scale), lo, min(lo + _BLOCK, total), M)
        k, f, A = k[counts], f[counts], A[counts]
        t = (j[None, :] - HALF) - f[:, None]
        v = A[:, None] * (0.5 * (1.0 + np.cos(2.0 * np.pi * t / WIDTH))) * np.sinc(t)
        n = k[:, None] - HALF + j[None, :] + WIDTH
        np.add.at(h, n.ravel(), v.ravel())
        if want_unit:
            np.add.at(cover, k - HALF + WIDTH, np.abs(A))
            np.add.at(cover, k - HALF + 2 * WIDTH, -np.abs(A))
    h = h[WIDTH:WIDTH + ntaps]
    if not want_unit:
        return h
    return h, np.maximum(np.cumsum(cover)[WIDTH:WIDTH + ntaps], 0.0) * 2.0 ** -24


def tap_unit(L, beta, src, mic, rate, ntaps, scale=1.0):
    """u[n] = 2^-24 sum |A_i| over the images whose 64-tap support covers tap n: one float32 rounding of every term that can
    reach the tap.  (A unit built from the windowed-sinc values themselves is useless: at the sinc's zero crossings a term's
    float32 error is thousands of times its own size.)"""
    return ism_rir(L, beta, src, mic, rate, ntaps, scale, want_unit=True)[1]


def _sinpi_f32(x):
    """sin(pi x) for float32 x in [0, 1], reduced to [0, 1/2] first (1 - x is exact there), as the device's sinpi is."""
    x = np.where(x > np.float32(0.5), np.float32(1.0) - x, x).astype(np.float32)
    return np.sin(np.float32(np.pi) * x, dtype=np.float32)


def ism_rir_f32(L, beta, src, mic, rate, ntaps, scale=1.0, drop_parity=None, drop_outer_axis=None, tap_shift=0, same_exponent=False):
    """sk_room_rirs' arithmetic in numpy -> h (ntaps,) float32.

    Geometry in fp64, exactly as in `_images` (no fused multiply-adds): the image's position, d, tau = d (rate / c), k = floor(tau),
    and A with integer powers by binary exponentiation.  From there on float32: f = fp32(tau - k), A32 = fp32(A), and for lane
    j = 0 .. 63 (tap n = k - 31 + j), with a_j = pi (j - 31) / 32 and cos a_j, sin a_j rounded from fp64 once,
        t = fp32(j - 31) - f;   w = 0.5 + 0.5 (cos a_j cos(pi f / 32) + sin a_j sin(pi f / 32));
        sinc = (-1)^j sinpi(f) / (pi t),  1 where t == 0;   h[n] += (A32 w) sinc.
    Summation order: image i belongs to chunk i >> 6, chunk c to wave c % 16; every wave adds its images, ascending, to an
    accumulator of its own, and h = acc0 + acc1 + ... + acc15 from the left.  The order is a function of the job's own arguments.  (The
    kernel's sinpi, cospi and reciprocal round differently from numpy's, and it may contract a product into the sum that follows:
    tests/test_gpu_room.py allows twice this function's own error for that.)

    The keyword switches each put ONE fault into the algorithm (one parity class left out; the outermost m of one axis that still
    holds an image left out; the tap index off by tap_shift; the exponent |m_a| used for both walls of an axis).
    tests/test_room.py uses them to show that its cases would catch such a fault; nothing else sets them."""
    L, beta, src, mic, rate, ntaps = _check(L, beta, src, mic, rate, ntaps)
    M = image_range(L, rate, ntaps)
    total = 8 * (2 * M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1)
    f32 = np.float32
    acc = np.zeros((WAVES, ntaps + 2 * WIDTH + 2), dtype=f32)
    j = np.arange(WIDTH, dtype=np.int64)
    tj = (j - HALF).astype(f32)
    cj = np.cos(np.pi * ((j - HALF) / 32.0)).astype(f32)
    sj = np.sin(np.pi * ((j - HALF) / 32.0)).astype(f32)
    sgn = np.where(j % 2 == 0, 1.0, -1.0).astype(f32)
    pi32 = f32(np.pi)
    outer = None
    if drop_outer_axis is not None:      # the largest |m_a| at which an image still counts (M_a itself carries a margin)
        a, outer = int(drop_outer_axis), 0
        for lo in range(0, total, _BLOCK):
            _, _, _, counts, m = _images(L, beta, src, mic, rate, ntaps, float(scale), lo, min(lo + _BLOCK, total), M, same_exponent)
            if counts.any():
                outer = max(outer, int(np.abs(m[a][counts]).max()))
    for lo in range(0, total, _BLOCK):
        hi = min(lo + _BLOCK, total)
        k, fr, A, counts, m = _images(L, beta, src, mic, rate, ntaps, float(scale), lo, hi, M, same_exponent)
        if drop_parity is not None:
            counts = counts & ((np.arange(lo, hi, dtype=np.int64) & 7) != int(drop_parity))
        if outer is not None:
            counts = counts & (np.abs(m[a]) != outer)
        wave = ((np.arange(lo, hi, dtype=np.int64) >> 6) % WAVES)[counts]
        k, f, A32 = k[counts], fr[counts].astype(f32), A[counts].astype(f32)
        cphi = np.cos(pi32 * (f * f32(1.0 / 32.0)), dtype=f32)
        sphi = np.sin(pi32 * (f * f32(1.0 / 32.0)), dtype=f32)
        s = _sinpi_f32(f)
        t = tj[None, :] - f[:, None]
        w = f32(0.5) + f32(0.5) * (cj[None, :] * cphi[:, None] + sj[None, :] * sphi[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            sinc = (sgn[None, :] * s[:, None]) * (f32(1.0) / (pi32 * t))
        sinc = np.where(t == f32(0.0), f32(1.0), sinc).astype(f32)
        v = ((A32[:, None] * w) * sinc).astype(f32)
        n = k[:, None] - HALF + j[None, :] + WIDTH + int(tap_shift)
        for wv in range(WAVES):
            pick = wave == wv
            np.add.at(acc[wv], n[pick].ravel(), v[pick].ravel())      # in index order, in float32: the wave's own order
    h = acc[0]
    for wv in range(1, WAVES):
        h = h + acc[wv]
    return h[WIDTH:WIDTH + ntaps].copy()


def eyring_beta(L, t60):
    """Six equal reflection coefficients for a NOMINAL reverberation time: Eyring's formula t60 = (24 ln 10 / c) V / (-S ln(1 -
    alpha)) solved for the absorption alpha, beta = sqrt(1 - alpha).

    t60 is a NOMINAL label, not the decay time of the RIRs this module makes: a rigid shoebox with uniform absorption is not a
    diffuse field.  The Schroeder (T20-based) decay time of such RIRs came out at 0.48 / 0.30 / 0.81 s for nominal 0.3 / 0.2 /
    0.5 s, 1.5 to 1.6 times the nominal.  It is not calibrated away here."""
    L = np.asarray(L, dtype=np.float64).reshape(-1)
    if L.shape != (3,) or not np.all(L > 0.0) or not float(t60) > 0.0:
        raise ValueError("eyring_beta: a room of three positive dimensions and t60 > 0 expected")
    V = float(L[0] * L[1] * L[2])
    S = 2.0 * float(L[0] * L[1] + L[1] * L[2] + L[0] * L[2])
    alpha = 1.0 - np.exp(-(24.0 * np.log(10.0) / C_SOUND) * V / (S * float(t60)))
    return np.full(6, np.sqrt(1.0 - alpha), dtype=np.float64)


def direct_delay(src, mic_ref, rate):
    """The direct path's delay at the reference microphone, floor(tau + 1/2) samples."""
    d = float(np.sqrt(np.sum((np.asarray(src, dtype=np.float64) - np.asarray(mic_ref, dtype=np.float64)) ** 2)))
    return int(np.floor(d * float(rate) / C_SOUND + 0.5))


def read_array(path_or_text):
    """An array geometry: C lines of `x y z`, metres from the array's centre, 1 <= C <= 8 (blank lines and `#` comments are
    skipped) -> (C, 3) float64.  A string with a line break, or one that names no file, is taken as the text itself."""
    import os
    text = str(path_or_text)
    name = text
    if "\n" not in text and os.path.exists(text):
        text = open(text).read()
    else:
        name = "the array text"
    rows = []
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        parts = line.split()
        try:
            row = [float(v) for v in parts]
        except ValueError:
            row = []
        if len(row) != 3 or not all(np.isfinite(row)):
            raise ValueError("%s: a microphone is a line of three numbers `x y z` in metres (got %r)" % (name, line))
        rows.append(row)
    if not 1 <= len(rows) <= MAX_MICS:
        raise ValueError("%s: %d microphones, 1..%d expected" % (name, len(rows), MAX_MICS))
    return np.array(rows, dtype=np.float64)


def draw_room(rng, dims_lo, dims_hi, t60_range, array, S, margin=0.5, min_dist=0.5, tries=100):
    """One room for one mixture, a function of rng (a numpy Generator) and the arguments alone -> a dict:
    'L' (3,) uniform in [dims_lo, dims_hi]; 't60' uniform in t60_range (nominal, see eyring_beta) and 'beta' = eyring_beta(L,
    t60); 'centre' (3,), the array's centre; 'yaw' uniform in [0, 2 pi), the array's rotation about the vertical; 'mics' (C, 3) =
    centre + R_yaw array; 'srcs' (S, 3).  The centre, every microphone and every source lie at least `margin` from every wall,
    every source at least `min_dist` from the centre.  Positions are redrawn up to `tries` times, then it is an error."""
    lo, hi = np.asarray(dims_lo, dtype=np.float64).reshape(-1), np.asarray(dims_hi, dtype=np.float64).reshape(-1)
    array = np.asarray(array, dtype=np.float64).reshape(-1, 3)
    if lo.shape != (3,) or hi.shape != (3,) or not np.all((lo > 0.0) & (lo <= hi)) or not 0.0 < float(t60_range[0]) <= float(t60_range[1]):
        raise ValueError("draw_room: 0 < dims_lo <= dims_hi (three numbers each) and 0 < t60_range[0] <= t60_range[1] expected")
    if not 1 <= len(array) <= MAX_MICS or int(S) < 1 or float(margin) <= 0.0 or float(min_dist) < MIN_DIRECT:
        raise ValueError("draw_room: 1..%d microphones, S >= 1, margin > 0 and min_dist >= %g expected" % (MAX_MICS, MIN_DIRECT))
    L = rng.uniform(lo, hi)
    t60 = float(rng.uniform(float(t60_range[0]), float(t60_range[1])))
    if np.any(L - 2.0 * margin <= 0.0):
        raise ValueError("draw_room: a room of %s m leaves nothing %g m from its walls" % (np.round(L, 2).tolist(), margin))

    def inside(x):
        return bool(np.all((x >= margin) & (x <= L - margin)))
    for _ in range(int(tries)):
        centre = rng.uniform(margin, L - margin)
        yaw = float(rng.uniform(0.0, 2.0 * np.pi))
        c, s = np.cos(yaw), np.sin(yaw)
        mics = centre + array @ np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
        if all(inside(x) for x in mics):
            break
    else:
        raise ValueError("draw_room: no place for the array %g m from the walls of a %s m room in %d tries"
                         % (margin, np.round(L, 2).tolist(), int(tries)))
    srcs = []
    for _ in range(int(S)):
        for _ in range(int(tries)):
            x = rng.uniform(margin, L - margin)
            if float(np.sqrt(np.sum((x - centre) ** 2))) >= min_dist and all(np.sqrt(np.sum((x - q) ** 2)) >= MIN_DIRECT for q in mics):
                srcs.append(x)
                break
        else:
            raise ValueError("draw_room: no place for a source %g m from the array in a %s m room in %d tries"
                             % (min_dist, np.round(L, 2).tolist(), int(tries)))
    return {'L': L, 't60': t60, 'beta': eyring_beta(L, t60), 'centre': centre, 'yaw': yaw, 'mics': mics, 'srcs': np.array(srcs)}
