"""A bit-faithful CPU restatement of what fir8_kernel (pymodem_amd/csrc/pm_fir8.hip) computes and decides, for the certified-bound tests.

Not a conftest and not a checker of values: it repeats, in numpy int64 / binary64 / x87 long double arithmetic, every step of the kernel
and of pm_fir8_plan_create that decides WHICH outputs the matrix pipe certifies, so that a test can (a) measure how close an input
brings the approximate sum y~ to the bound E the kernel uses and (b) predict the exact number of outputs the kernel flags for
fir8_exact_kernel (pm_fir8_rows_signs_f64's `h_recomputed`, one per flagged output).

  plan    S = 22 - e(max|h|), q = rint(h 2^S), three balanced base-256 digits; c1 = (sum|h 2^S - q| + 1.01 (m+1) u sum|h| 2^S) * 1.000001
          and c2 = (0.75 sum|q| + 128 (sum|q_0| + 256 (sum|q_0| + sum|q_1|))) * 1.000001, summed in long double in tap order, as the
          host does.
  window  8192 outputs per workgroup; the workgroup reads samples wg0 .. wg0 + 8192 + 64 * 4J - 1 (the rows API: none past n).
          hm = the largest binary32 bit pattern of |x| in the window; e = ((hm + 1) >> 23) - 126, Xmax = binary32(hm + 1), s2 = 22 - e.
          hm >= pattern(2^100) or hm < pattern(2^-100): no matrix pipe -- all zeros: every bit set, nothing flagged; else all flagged.
  samples X = rint(binary32(x) 2^s2) (half to even), three balanced digits.
  sums    W_w = sum_t sum_{i+j=w} q_j[m-1-t] x_i[k+t] for w = 2, 3, 4 (the six products kept), val = W_2 + 256 W_3 + 65536 W_4,
          y~ = val 65536 2^-(S+s2).
  bound   Eint = ceil((c1 (Xmax 2^s2) + c2) (1 + 1e-9) / 65536) + 1, in units of 65536 2^-(S+s2); flagged = !(|val| > Eint).
"""
import numpy as np

KWG_OUT = 8192
U = 1.1102230246251565e-16
_LO, _HI = 0x0D800000, 0x71800000                   # binary32 patterns of 2^-100 and 2^100


def digits(v):
    """Three balanced base-256 digits of int64 values (|v| <= 2^23): d = ((v + 128) & 255) - 128, v = (v - d) / 256."""
    v = np.asarray(v, dtype=np.int64).copy()
    out = []
    for _ in range(3):
        d = ((v + 128) & 255) - 128
        out.append(d)
        v = (v - d) // 256
    assert not v.any(), "a value does not fit three digits"
    return out


class Plan:
    """pm_fir8_plan_create for taps h."""

    def __init__(self, h):
        h = np.ascontiguousarray(h, dtype=np.float64)
        m = len(h)
        assert m >= 1 and m + 15 <= 1024 and np.isfinite(h).all()
        hmax = float(np.abs(h).max())
        assert hmax > 0.0
        e = int(np.frexp(hmax)[1])
        self.m, self.h = m, h
        self.S = S = 22 - e
        self.J = ((m + 15 + 63) // 64 + 3) // 4
        scaled = np.ldexp(h, S)
        self.q = q = np.rint(scaled).astype(np.int64)
        self.delta = scaled - q                                     # exact: |scaled| < 2^23
        self.qd = digits(q)
        L = np.longdouble
        seq = lambda a: np.cumsum(np.asarray(a, dtype=L))[-1]       # left to right in long double, as the host loop adds
        tapq = seq(np.abs(self.delta))
        qabs = seq(np.abs(q))
        d0abs, d1abs = seq(np.abs(self.qd[0])), seq(np.abs(self.qd[1]))
        habs = seq(np.abs(h))
        f = L("1.000001")
        self.c1 = float((tapq + L("1.01") * L(m + 1) * L(U) * np.ldexp(habs, S)) * f)
        self.c2 = float((L("0.75") * qabs + L(128.0) * (d0abs + L(256.0) * (d0abs + d1abs))) * f)
        self.window = KWG_OUT + 64 * 4 * self.J
        # the reversed taps' digits, as the band table holds them: output k = sum_t q[m-1-t] X[k+t]
        self.qr = [d[::-1].copy() for d in self.qd]

    def scale_of(self, xmax_bits):
        """(e, s2, Xmax) for the window's largest pattern hm."""
        e = ((int(xmax_bits) + 1) >> 23) - 126
        mx = float(np.array([int(xmax_bits) + 1], dtype=np.uint32).view(np.float32)[0])
        return e, 22 - e, mx

    def eint(self, mx, s2):
        return np.ceil((self.c1 * (mx * np.ldexp(1.0, s2)) + self.c2) * (1.0 + 1e-9) * (1.0 / 65536.0)) + 1.0

    def run(self, x):
        """One row x (n >= m) -> dict of per-output arrays (nout = n - m + 1):
        yt    y~ (NaN where the workgroup took no matrix pipe), E the bound the kernel compares with (Eint in value units),
        Ebound the bound of the source comment before rounding up ((c1 Xmax + c2 2^-s2) 2^-S), flagged, sign (the kernel's bit where
        not flagged)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, m = len(x), self.m
        nout = n - m + 1
        assert nout >= 1
        yt, E, Eb = np.full(nout, np.nan), np.full(nout, np.nan), np.full(nout, np.nan)
        flagged, sign = np.zeros(nout, bool), np.zeros(nout, bool)
        for wg0 in range(0, nout, KWG_OUT):
            k1 = min(wg0 + KWG_OUT, nout)
            win = x[wg0:min(wg0 + self.window, n)]
            with np.errstate(over="ignore", invalid="ignore"):
                f32 = win.astype(np.float32)
            hm = int((f32.view(np.uint32) & np.uint32(0x7FFFFFFF)).max())
            if hm >= _HI or hm < _LO:
                zeros = bool((win == 0.0).all())
                flagged[wg0:k1] = not zeros
                sign[wg0:k1] = zeros
                if zeros:
                    yt[wg0:k1] = 0.0
                continue
            _, s2, mx = self.scale_of(hm)
            X = np.rint(f32.astype(np.float64) * np.ldexp(1.0, s2)).astype(np.int64)
            xd = digits(X)
            cnt = k1 - wg0
            W = [np.zeros(cnt, np.int64) for _ in range(3)]
            for i in range(3):
                sw = np.lib.stride_tricks.sliding_window_view(xd[i], m)[:cnt]
                for j in range(3):
                    if i + j >= 2:
                        W[i + j - 2] += sw @ self.qr[j]
            val = W[0] + 256 * W[1] + 65536 * W[2]
            assert np.abs(val).max(initial=0) < 2 ** 42
            vf = val.astype(np.float64)
            ei = self.eint(mx, s2)
            unit = np.ldexp(65536.0, -(self.S + s2))
            yt[wg0:k1] = vf * unit
            E[wg0:k1] = ei * unit
            Eb[wg0:k1] = (self.c1 * mx + self.c2 * np.ldexp(1.0, -s2)) * np.ldexp(1.0, -self.S)
            flagged[wg0:k1] = ~(np.abs(vf) > ei)
            sign[wg0:k1] = vf > 0.0
        return {"yt": yt, "E": E, "Ebound": Eb, "flagged": flagged, "sign": sign}

    def quantise(self, x, s2):
        """X = rint(binary32(x) 2^s2), the integer the kernel multiplies (for generators that aim at particular digits)."""
        return np.rint(np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64) * np.ldexp(1.0, s2)).astype(np.int64)


def adversarial_rows(plan, targets, directions, fir_canon, xmax=1023.0):
    """One row of m samples (ONE output) per target: every error term of the bound lined up with its worst case, then the canonical sum
    steered onto the target by one free sample.

    For the sample at position t (tap q[m-1-t] =: q, its digits q_0, q_1, and delta = h 2^S - q), with direction sigma = +-1 (the sign
    y~ - y should take), the error in units of 2^-(S+s2) is
        -(x_0 (q_0 + 256 q_1) + 256 x_1 q_0)  -  delta x 2^s2  +  q r,      r = X - x 2^s2 (the sample's rounding),
    so: x_0 = -128 or 126 (even, for the tie below) against the sign of sigma (q_0 + 256 q_1); x_1 = -128 or 127 against sigma q_0;
    x_2 = +-63 (|x| near Xmax) against sigma delta; and x 2^s2 = X - r with r = sigma sign(q) (1/2 + 3/8 of a binary32 unit): binary32
    rounds it to X -+ 1/2 and rint (half to even) to X.  The sample at the smallest |h| pins Xmax (`xmax`: the workgroup's scale); the
    x_2 of the larger of the two signed groups of h x is scaled down so that the row sums to about zero, and the sample at the largest
    |h| then carries the sum to its target (two corrections against the canonical sum `fir_canon`).
    -> (rows (R, m), the free sample's index)"""
    m = plan.m
    hr = plan.h[::-1]
    qr, dr = plan.q[::-1], plan.delta[::-1]
    q0, q1 = plan.qr[0], plan.qr[1]
    hm = int(np.array([xmax], np.float32).view(np.uint32)[0])
    _, s2, _ = plan.scale_of(hm)
    free, pin = int(np.argmax(np.abs(hr))), int(np.argmin(np.abs(hr)))
    sgn = lambda v: np.where(v >= 0, 1, -1)
    base = {}
    for sigma in (1, -1):
        x0 = np.where(-sigma * sgn(q0 + 256 * q1) > 0, 126, -128)
        x1 = np.where(-sigma * sgn(q0) > 0, 127, -128)
        s = -sigma * sgn(dr)
        x2 = np.full(m, 63)
        X = lambda: x0 + 256 * x1 + 65536 * s * x2
        c = hr * X().astype(np.float64)
        c[[free, pin]] = 0.0
        P, N = c[c > 0].sum(), -c[c < 0].sum()
        big = (c > 0) if P > N else (c < 0)
        x2 = np.where(big, np.maximum(1, np.rint(63 * min(P, N) / max(P, N))).astype(np.int64), x2)
        # greedy: the largest taps first, one step of |x_2| each where it brings the sum nearer zero
        for t in np.argsort(-np.abs(hr)):
            if t in (free, pin):
                continue
            R = float(np.dot(np.delete(hr, [free, pin]), np.delete(X(), [free, pin]).astype(np.float64)))
            step = hr[t] * 65536.0 * s[t]
            k = int(np.clip(np.rint(R / step), x2[t] - 63, x2[t] - 1))
            if k != 0 and abs(R - k * step) < abs(R):
                x2[t] -= k
        Xi = X()
        ulp = np.spacing(np.abs(Xi).astype(np.float32) * np.float32(2.0 ** -s2)).astype(np.float64) * 2.0 ** s2
        r = sigma * sgn(qr) * (0.5 + 0.375 * ulp)
        x = (Xi - r) * 2.0 ** -s2
        bad = plan.quantise(x, s2) != Xi                     # (binary32 could not take the fraction: no rounding error there)
        x[bad] = Xi[bad] * 2.0 ** -s2
        x[pin], x[free] = xmax, 0.0
        assert np.array_equal(plan.quantise(np.delete(x, [free, pin]), s2), np.delete(Xi, [free, pin]))
        base[sigma] = x
    rows = np.stack([base[1 if d > 0 else -1] for d in directions])
    for _ in range(2):
        y = np.array([fir_canon(r, plan.h)[0] for r in rows])
        rows[:, free] = np.clip(rows[:, free] + (np.asarray(targets) - y) / hr[free], -0.98 * xmax, 0.98 * xmax)
    return rows, free


def window_taps(m, rng):
    """A matched-filter-like shape (as tests/test_gpu_fir8.py draws them): windowed sinc, L2-normalised, a little asymmetry."""
    t = np.arange(m) - (m - 1) / 2
    h = np.sinc(t / (m / 12.0)) * np.hanning(m + 2)[1:-1] + 1e-3 * rng.standard_normal(m)
    return h / np.linalg.norm(h)


def tap_sets():
    """The modems' own filters (BPSK 300: 961 taps, QPSK 2400: 241) and lengths at the edges of the band's blocks (J = 1, 2, 3, 4)."""
    from pymodem_amd import chain_builder as cb
    out = []
    for kind, cfg in (("bpsk", "300"), ("mpsk", "qpsk_2400")):
        md = cb.ModemConfigurator(48000, {"type": kind, "config": cfg, "options": {}})
        out.append((f"{kind}_{cfg}", np.asarray(md.rrc_taps, dtype=np.float64)))
    for m in (16, 497, 498, 1009):
        out.append((f"m{m}", window_taps(m, np.random.default_rng(m))))
    return out


def adversarial_cases(fir_canon, per_direction=120):
    """[(name, plan, rows, directions)]: per tap set, targets for the canonical sum swept evenly over [-2E, 2E], each once with the
    error pushed up and once down."""
    out = []
    for name, h in tap_sets():
        plan = Plan(h)
        E = plan.run(np.full(plan.m, 1023.0))["Ebound"][0]
        targets = np.tile(np.linspace(-2.0 * E, 2.0 * E, per_direction), 2)
        dirs = np.repeat([1, -1], per_direction)
        rows, _ = adversarial_rows(plan, targets, dirs, fir_canon)
        out.append((name, plan, rows, dirs))
    return out
