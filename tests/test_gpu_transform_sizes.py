"""Every transform size the compat surface accepts, through the FFTW names (include/ka9q_hip_fftw.h), against numpy's float64
transforms: all even 2^a 3^b 5^c 7^d up to 65536 as c2c forward, c2c backward, r2c and c2r, and the powers of two from 2^17 to
2^22 as c2c.

Sizes up to 16384 run in one LDS block (k_fft_single: lds_fft for a power of two, lds_fft_mixed otherwise); larger ones are
split N = na x nb through device memory (launch_fft_large): a power of two into two powers of two, any other N by the rule
restated in _split below, which leaves either side a power of two, a mixed size or an odd one.  Each of those is a different
path through fft_any and the inter-pass twiddles, so the sweep names the class of every size and checks that no class is empty.

(This module sorts after test_gpu_compat.py on purpose: the plans of 488 mixed sizes leave some 80 MB of tables on the device,
which are never freed, and that module's memory test should not meet them half way.)"""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from test_oracle_filter import _as

pytestmark = pytest.mark.gpu

C2C_TOL = 5e-7      # relative RMS; the project's bounds, met at 65536, 48000 and 47040 points (test_gpu_compat.py)
R2C_TOL = 4e-7


@pytest.fixture(scope="module")
def lib(gpu):
    L = kq.load_library()
    for n in ("fftwf_alloc_real", "fftwf_alloc_complex"):
        getattr(L, n).restype = C.c_void_p
        getattr(L, n).argtypes = [C.c_size_t]
    L.fftwf_free.argtypes = [C.c_void_p]
    L.fftwf_plan_dft_1d.restype = C.c_void_p
    L.fftwf_plan_dft_1d.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint]
    L.fftwf_plan_dft_r2c_1d.restype = C.c_void_p
    L.fftwf_plan_dft_r2c_1d.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint]
    L.fftwf_plan_dft_c2r_1d.restype = C.c_void_p
    L.fftwf_plan_dft_c2r_1d.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint]
    L.fftwf_execute.argtypes = [C.c_void_p]
    L.fftwf_destroy_plan.argtypes = [C.c_void_p]
    return L


def _radices(n):
    """fft_dim's rule: 4s first, then 2, 3s, 5s, 7s"""
    f = []
    for r in (4, 2, 3, 5, 7):
        while n % r == 0:
            f.append(r)
            n //= r
    assert n == 1
    return f


def _pow2(n):
    return n & (n - 1) == 0


def _split(n):
    """-> (na, nb, class) of an n-point transform.  Beyond one LDS block a power of two splits into 2^ceil(log2 n / 2) and the
    rest; any other n multiplies its radices, in fft_dim's order, into na while na^2 < n."""
    if n <= 16384:
        return n, 1, "one LDS block, " + ("power of two" if _pow2(n) else "mixed")
    if _pow2(n):
        na = 1 << ((n.bit_length() - 1 + 1) // 2)
        return na, n // na, "large, power of two x power of two"
    na = 1
    for r in _radices(n):
        if na * na < n:
            na *= r
    nb = n // na
    kind = lambda m: "power of two" if _pow2(m) else "odd" if m & 1 else "mixed"      # noqa: E731
    return na, nb, "large, %s x %s" % (kind(na), kind(nb))


def _smooth_even(limit):
    out = []
    for n in range(2, limit + 1, 2):
        m = n
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            out.append(n)
    return out


SIZES = _smooth_even(65536)


def test_the_sweep_reaches_every_class_of_size():
    """Host arithmetic only: the sizes, their splits and their classes as the sweep below names them."""
    assert len(SIZES) == 498 and sum(1 for n in SIZES if n <= 16384) == 317
    classes = {}
    for n in SIZES:
        na, nb, cls = _split(n)
        assert na * nb == n and na <= 16384 and nb <= 16384, (n, na, nb)
        # FftDim::f holds 12 radices; the longest plan is 2 x 3^9 = 39366
        assert all(_pow2(m) or len(_radices(m)) <= 10 for m in (n, na, nb)), (n, na, nb)
        classes.setdefault(cls, []).append(n)
    for cls, members in sorted(classes.items()):
        print("%-40s %3d sizes, %d ... %d" % (cls, len(members), members[0], members[-1]))
    large = [n for n in SIZES if n > 16384 and not _pow2(n)]
    assert len(large) == 179
    assert sum(1 for n in large if _split(n)[1] & 1) == 151
    for cls in ("one LDS block, power of two", "one LDS block, mixed", "large, mixed x odd", "large, power of two x mixed",
                "large, power of two x odd"):
        assert classes.get(cls), cls
    # a power-of-two first factor inside a mixed N: lds_fft on the next power of two's table, inter-pass twiddles from N's own
    first_pow2 = [n for n in large if _pow2(_split(n)[0])]
    print("power-of-two first factor inside a mixed N: %d sizes" % len(first_pow2))
    assert len(first_pow2) >= 24 and {17920, 18432, 19200, 20480, 24576} <= set(first_pow2)


def _err(a, b):
    return np.sqrt(np.mean(np.abs(a - b) ** 2) / np.mean(np.abs(b) ** 2))


def _run(lib, kind, n, rng):
    """one transform of n points -> (relative RMS error against float64, bound)"""
    if kind in ("c2c_forward", "c2c_backward"):
        sign = -1 if kind == "c2c_forward" else +1
        a, b = lib.fftwf_alloc_complex(n), lib.fftwf_alloc_complex(n)
        plan = lib.fftwf_plan_dft_1d(n, a, b, sign, 1 << 6)
        assert plan, n
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        _as(a, n, np.complex64)[:] = x
        _as(b, n, np.complex64)[:] = 0
        lib.fftwf_execute(plan)
        ref = np.fft.fft(x.astype(np.complex128)) if sign < 0 else np.fft.ifft(x.astype(np.complex128)) * n
        e, tol = _err(_as(b, n, np.complex64), ref), C2C_TOL
    elif kind == "r2c":
        a, b = lib.fftwf_alloc_real(n), lib.fftwf_alloc_complex(n // 2 + 1)
        plan = lib.fftwf_plan_dft_r2c_1d(n, a, b, 1 << 6)
        assert plan, n
        x = rng.standard_normal(n).astype(np.float32)
        _as(a, n, np.float32)[:] = x
        _as(b, n // 2 + 1, np.complex64)[:] = 0
        lib.fftwf_execute(plan)
        e, tol = _err(_as(b, n // 2 + 1, np.complex64), np.fft.rfft(x.astype(np.float64))), R2C_TOL
    else:
        # c2r of a real signal's own spectrum, as y / n against x; held to the c2c bound (it is one complex transform of the
        # Hermitian-extended bins).  The bins go in as float32: x is compared with what float64 makes of those very bins.
        a, b = lib.fftwf_alloc_complex(n // 2 + 1), lib.fftwf_alloc_real(n)
        plan = lib.fftwf_plan_dft_c2r_1d(n, a, b, 1 << 6)
        assert plan, n
        X = np.fft.rfft(rng.standard_normal(n)).astype(np.complex64)
        _as(a, n // 2 + 1, np.complex64)[:] = X
        _as(b, n, np.float32)[:] = 0
        lib.fftwf_execute(plan)
        x = np.fft.irfft(X.astype(np.complex128), n)     # (ignores the imaginary parts of DC and Nyquist, as FFTW's c2r)
        e, tol = _err(_as(b, n, np.float32).astype(np.float64) / n, x), C2C_TOL
    lib.fftwf_destroy_plan(plan)
    lib.fftwf_free(a)
    lib.fftwf_free(b)
    return e, tol


@pytest.mark.parametrize("kind", ["c2c_forward", "c2c_backward", "r2c", "c2r"])
def test_every_even_7_smooth_size_up_to_65536(lib, kind):
    rng = np.random.default_rng(len(kind))
    worst, bad = {}, []
    for n in SIZES:
        na, nb, cls = _split(n)
        e, tol = _run(lib, kind, n, rng)
        if e > worst.get(cls, (0.0, 0))[0]:
            worst[cls] = (e, n)
        if not e < tol:
            bad.append("n = %d (%d x %d; %s): %.3g" % (n, na, nb, cls, e))
    for cls, (e, n) in sorted(worst.items()):
        print("%-12s %-40s worst %.3g at n = %d" % (kind, cls, e, n))
    assert not bad, "%s: %d of %d sizes beyond the bound:\n%s" % (kind, len(bad), len(SIZES), "\n".join(bad))


@pytest.mark.parametrize("sign", [-1, +1])
@pytest.mark.parametrize("log2n", range(17, 23))
def test_powers_of_two_beyond_65536(lib, log2n, sign):
    """Two passes of up to 2048 points each through device memory.  The bound is the 65536-point one grown with the pass count:
    5e-7 log2(n) / 16."""
    n = 1 << log2n
    e, _ = _run(lib, "c2c_forward" if sign < 0 else "c2c_backward", n, np.random.default_rng(log2n))
    na, nb, cls = _split(n)
    print("n = 2^%d (%d x %d) sign %+d: %.3g (bound %.3g)" % (log2n, na, nb, sign, e, C2C_TOL * log2n / 16))
    assert e < C2C_TOL * log2n / 16, (n, na, nb, cls, e)
