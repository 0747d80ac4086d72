"""The modulator bank (kq_mod_*, ka9q_sdr_amd/csrc/kq_mod.hip) on the GPU against the CPU model of tests/mod_model.py,
against the library's own compat filter API run as modulate.c's loop, and end to end through the receiver bank."""
import ctypes as C

import numpy as np
import pytest

import ka9q_sdr_amd as kq
from ka9q_sdr_amd.modulate import KQ_PCM_S16, StationConfig
from common import rel_rms
import mod_model as mm

pytestmark = pytest.mark.gpu

REF = dict(samprate=192000, L=4096, M=4097, interp=4)        # modulate.c:25,109-112
WIDE = dict(samprate=10000000, L=8192, M=8193, interp=256)   # 10 MS/s, 39.0625 kHz audio
G240 = dict(samprate=240000, L=4800, M=4801, interp=5)       # N = 9600 = 2^7 3 5^2, 48 kHz audio


def _cfg(st):
    return StationConfig(st["mod_type"], st["low"], st["high"], st["carrier"], st["kaiser_beta"], st["deviation"],
                         st["frequency"], st["sweep"], st["amplitude_dbfs"])


def _audio(rng, rows, n, rate, scale=0.5):
    """speech-band test audio: two tones per row plus a little noise, as int16 (modulate.c reads int16)"""
    t = np.arange(n) / rate
    f1 = rng.uniform(300, 2500, (rows, 1))
    f2 = rng.uniform(300, 2500, (rows, 1))
    x = scale * (0.6 * np.sin(2 * np.pi * f1 * t) + 0.3 * np.sin(2 * np.pi * f2 * t + 1.0)) + 0.02 * rng.standard_normal((rows, n))
    return np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)


def _scaled(pcm16):
    return pcm16.astype(np.float32) * np.float32(1.0 / 32767)   # modulate.c:23,141


def _check_s16(got, want_cf):
    d = np.abs(got.astype(np.int32) - mm.to_s16(want_cf).astype(np.int32))
    assert d.max() <= 1, d.max()


@pytest.mark.parametrize("mode,sweep", [("am", 0.0), ("usb", 0.0), ("lsb", 0.0), ("ame", 0.0), ("am", 1234.5)])
def test_one_station_at_modulate_defaults(gpu, mode, sweep):
    g = REF
    nblocks = 8
    rng = np.random.default_rng(3)
    pcm = _audio(rng, 3, nblocks * g["L"] // g["interp"], g["samprate"] / g["interp"])
    st = mm.station(mode, sweep=sweep)
    ref = mm.OracleStation(g["samprate"], g["L"], g["M"], g["interp"], st)
    a = _scaled(pcm[2])
    La = g["L"] // g["interp"]
    want = np.concatenate([ref.block(a[b * La:(b + 1) * La]) for b in range(nblocks)])
    bank = kq.ModBank(max_stations=3, max_blocks=8, **g)
    bank.set_station(2, _cfg(st))
    got, s16 = bank.process(pcm, nblocks)
    bank.close()
    assert rel_rms(got, want) <= 1e-5
    _check_s16(s16.reshape(-1, 2), want)


class CompatOsc(C.Structure):   # struct osc of ka9q_hip_compat.h
    _fields_ = [("freq", C.c_double), ("rate", C.c_double), ("phasor", C.c_double * 2), ("phasor_step", C.c_double * 2),
                ("phasor_step_step", C.c_double * 2), ("mutex", C.c_byte * 40), ("steps", C.c_int)]


class _Cd(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


def test_one_station_against_compat_loop(gpu):
    """modulate.c:109-163 run in ctypes on the library's own create_filter_input / create_filter_output / window_filter /
    set_osc / step_osc: a second GPU path to the same numbers"""
    from test_gpu_compat import FilterIn, FilterOut
    L = kq.load_library()
    L.create_filter_input.restype = C.POINTER(FilterIn)
    L.create_filter_input.argtypes = [C.c_uint, C.c_uint, C.c_int]
    L.create_filter_output.restype = C.POINTER(FilterOut)
    L.create_filter_output.argtypes = [C.POINTER(FilterIn), C.c_void_p, C.c_uint, C.c_int]
    L.execute_filter_input.argtypes = [C.POINTER(FilterIn)]
    L.execute_filter_output.argtypes = [C.POINTER(FilterOut)]
    L.delete_filter_input.argtypes = [C.POINTER(FilterIn)]
    L.delete_filter_output.argtypes = [C.POINTER(FilterOut)]
    L.window_filter.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float]
    L.set_osc.argtypes = [C.POINTER(CompatOsc), C.c_double, C.c_double]
    L.step_osc.argtypes = [C.POINTER(CompatOsc)]
    L.step_osc.restype = _Cd
    g = REF
    Fs, Lb, M, I = g["samprate"], g["L"], g["M"], g["interp"]
    N = Lb + M - 1
    nblocks = 8
    st = mm.station("usb", frequency=-31000.0, sweep=-700.0, amplitude_dbfs=-12.0)
    pcm = _audio(np.random.default_rng(9), 1, nblocks * Lb // I, Fs / I)
    libc = C.CDLL(None)
    libc.malloc.restype = C.c_void_p
    resp = mm.target_response(Fs, Lb, M, I, st["low"], st["high"])
    p = libc.malloc(8 * N)
    C.memmove(p, resp.ctypes.data, 8 * N)
    assert L.window_filter(Lb, M, p, 3.0) == 0                      # modulate.c:130
    fi = L.create_filter_input(Lb, M, 3)                            # REAL
    fo = L.create_filter_output(fi, p, 1, 1)                        # decimate 1, COMPLEX
    osc = CompatOsc()
    L.set_osc(C.byref(osc), st["frequency"] / Fs, st["sweep"] / (float(Fs) * Fs))
    amp = 10 ** (st["amplitude_dbfs"] / 20)
    a = _scaled(pcm[0])
    want = []
    for b in range(nblocks):
        x = np.zeros(Lb, np.float32)
        x[::I] = a[b * Lb // I:(b + 1) * Lb // I]
        mm._as(fi.contents.input, Lb, np.float32)[:] = x
        assert L.execute_filter_input(fi) == 0 and L.execute_filter_output(fo) == 0
        y = mm._as(fo.contents.output, Lb, np.complex64).astype(np.complex128)
        ph = np.array([complex(z.re, z.im) for z in (L.step_osc(C.byref(osc)) for _ in range(Lb))])
        want.append((y * ph * amp).astype(np.complex64))
    want = np.concatenate(want)
    L.delete_filter_output(fo)
    L.delete_filter_input(fi)
    bank = kq.ModBank(max_stations=1, max_blocks=4, **g)
    bank.set_station(0, _cfg(st))
    got = np.concatenate([bank.process(pcm[:, h * 4 * Lb // I:], 4, want_s16=False)[0] for h in range(2)])
    bank.close()
    assert rel_rms(got, want) <= 1e-5


def _mixed_plan(rng, n, g, fm_every=5):
    Fs = g["samprate"]
    kinds = ["am", "usb", "lsb", "ame"]
    plan = []
    for s in range(n):
        mode = "fm" if s % fm_every == 4 else kinds[s % 4]
        f = rng.uniform(-0.45, 0.45) * Fs
        sweep = rng.uniform(-2000, 2000) if s % 7 == 3 else 0.0
        plan.append(mm.station(mode, frequency=float(f), sweep=float(sweep), amplitude_dbfs=float(rng.uniform(-50, -40))))
    return plan


@pytest.mark.parametrize("geom", [WIDE, G240], ids=["10MSps", "240k"])
def test_bank_of_1024_stations(gpu, geom):
    g = geom
    S, nblocks = 1024, 4
    rng = np.random.default_rng(11)
    plan = _mixed_plan(rng, S, g)
    pcm = _audio(rng, S, nblocks * g["L"] // g["interp"], g["samprate"] / g["interp"])
    model = mm.BankModel(**g)
    bank = kq.ModBank(max_stations=S, max_blocks=nblocks, **g)
    for s, st in enumerate(plan):
        model.set_station(s, st)
        bank.set_station(s, _cfg(st))
    want, each = model.process(_scaled(pcm), nblocks, per_station=True)
    got, s16 = bank.process(pcm, nblocks)
    assert rel_rms(got, want) <= 1e-5
    _check_s16(s16, want)
    bank.close()
    # the FM stations alone (their phase is a running sum: held to 5e-5)
    fm = [s for s, st in enumerate(plan) if st["mod_type"] == 1]
    bank = kq.ModBank(max_stations=S, max_blocks=nblocks, **g)
    for s in fm:
        bank.set_station(s, _cfg(plan[s]))
    got, _ = bank.process(pcm, nblocks, want_s16=False)
    bank.close()
    assert rel_rms(got, sum(each[s] for s in fm)) <= 5e-5


def test_determinism(gpu):
    g = WIDE
    S, nblocks = 300, 4
    rng = np.random.default_rng(5)
    plan = _mixed_plan(rng, S, g, fm_every=3)
    pcm = _audio(rng, S, nblocks * g["L"] // g["interp"], g["samprate"] / g["interp"])
    La = g["L"] // g["interp"]

    def run(per_call):
        bank = kq.ModBank(max_stations=S, max_blocks=nblocks, **g)
        for s, st in enumerate(plan):
            bank.set_station(s, _cfg(st))
        outs = [bank.process(np.ascontiguousarray(pcm[:, c * La:(c + per_call) * La]), per_call)
                for c in range(0, nblocks, per_call)]
        bank.close()
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])

    a, b, c = run(nblocks), run(nblocks), run(1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


def test_control_between_calls(gpu):
    g = WIDE
    S, nb = 40, 2
    La = g["L"] // g["interp"]
    rng = np.random.default_rng(21)
    plan = _mixed_plan(rng, S, g, fm_every=4)
    pcm = _audio(rng, S, 5 * nb * La, g["samprate"] / g["interp"])
    model = mm.BankModel(**g)
    bank = kq.ModBank(max_stations=64, max_blocks=nb, **g)
    for s in range(0, S, 2):
        model.set_station(s, plan[s])
        bank.set_station(s, _cfg(plan[s]))
    steps = [
        lambda: None,
        lambda: [(model.set_station(s, plan[s]), bank.set_station(s, _cfg(plan[s]))) for s in range(1, S, 2)],   # add
        lambda: [(model.remove_station(s), bank.remove_station(s)) for s in range(0, S, 6)],                      # remove
        lambda: [(model.set_station(s, dict(plan[s], frequency=plan[s]["frequency"] + 12345.6, amplitude_dbfs=-41.0)),
                  bank.set_station(s, _cfg(dict(plan[s], frequency=plan[s]["frequency"] + 12345.6, amplitude_dbfs=-41.0))))
                 for s in range(1, S, 4)],                                                                          # retune
        lambda: [(model.set_station(s, mm.station("fm" if plan[s]["mod_type"] == 0 else "lsb", frequency=plan[s]["frequency"])),
                  bank.set_station(s, _cfg(mm.station("fm" if plan[s]["mod_type"] == 0 else "lsb", frequency=plan[s]["frequency"]))))
                 for s in range(3, S, 4)],                                                                          # mode
    ]
    for k, step in enumerate(steps):
        step()
        chunk = np.ascontiguousarray(pcm[:, k * nb * La:(k + 1) * nb * La])
        want, _ = model.process(_scaled(chunk), nb)
        got, s16 = bank.process(chunk, nb)
        assert rel_rms(got, want) <= 5e-5, k
        _check_s16(s16, want)
    bank.close()


def test_argument_errors_with_a_bank(gpu):
    bank = kq.ModBank(max_stations=4, max_blocks=2, **REF)
    with pytest.raises(kq.KqError, match="max_stations"):
        bank.set_station(4, _cfg(mm.station()))
    with pytest.raises(kq.KqError, match="holds no station"):
        bank.remove_station(1)
    bank.set_station(2, _cfg(mm.station()))
    with pytest.raises(ValueError, match="slot 2"):   # host rows 0 .. 2 are read: two rows are too few
        bank.process(np.zeros((2, 1024), np.int16), 1)
    lib = bank.lib
    assert lib.kq_mod_process(bank.h, None, 5, 0, 1, 0, None, None) == -1
    assert b"pcm_format" in lib.kq_last_error()
    bank.close()
    # the AFSK decoder keeps refusing the new host-order int16 format
    afsk = kq.AfskBank(1, 4)
    x = np.zeros(1000, np.int16)
    assert afsk.L.kq_afsk_push(afsk.h, x.ctypes.data, KQ_PCM_S16, 1, 1000, 1000, 0) == -1
    afsk.close()


def _tone_db(audio, rate, tone, lo_hz=0.0):
    """-> (peak bin, tone bin, tone-to-residual dB) of one channel's audio, bins below lo_hz left out"""
    x = np.asarray(audio, np.float64)
    x = x - x.mean()
    P = np.abs(np.fft.rfft(x * np.hanning(len(x)))) ** 2
    k = int(round(tone * len(x) / rate))
    lo = max(1, int(np.ceil(lo_hz * len(x) / rate)))
    peak = int(np.argmax(P[lo:])) + lo
    sig = P[max(k - 4, lo):k + 5].sum()
    res = P[lo:].sum() - sig
    return peak, k, 10 * np.log10(sig / max(res, 1e-30))


def _loopback(calls=8):
    """64 stations synthesised at 10 MS/s, int16 into a kq_bank (D = 256) with one channel per station in the matching
    mode.  -> dict: per-station audio [blocks][olen] and receiver status [blocks], tones, mode names, audio rate, and the
    relative RMS error of the synthesised cf32 stream against the model (BankModel) over every call"""
    g = WIDE
    Fs, Lb, M, I = g["samprate"], g["L"], g["M"], g["interp"]
    rate = Fs / I
    S, per_call = 64, 8
    nblocks = per_call * calls
    kinds = [("am", 1000.0, dict(demod_type=kq.KQ_AM_DEMOD, low=-5000.0, high=5000.0)),
             ("usb", 700.0, dict(demod_type=kq.KQ_LINEAR_DEMOD, low=50.0, high=3000.0)),
             ("lsb", 1900.0, dict(demod_type=kq.KQ_LINEAR_DEMOD, low=-3000.0, high=-50.0)),
             ("fm", 1000.0, dict(demod_type=kq.KQ_FM_DEMOD, low=-8000.0, high=8000.0))]
    mod = kq.ModBank(max_stations=S, max_blocks=per_call, **g)
    model = mm.BankModel(**g)
    rx = kq.Bank(Fs, Lb, M, 256, S, per_call)
    n = nblocks * Lb // I
    t = np.arange(n) / rate
    pcm = np.zeros((S, n), np.int16)
    tones, names = [], []
    for s in range(S):
        mode, tone, rcfg = kinds[s % 4]
        f = -4.0e6 + s * 125000.0 + 1234.5
        st = mm.station(mode, frequency=f, amplitude_dbfs=-42.0, deviation=3000.0)
        mod.set_station(s, _cfg(st))
        model.set_station(s, st)
        pcm[s] = np.round(0.5 * np.sin(2 * np.pi * tone * t) * 32767).astype(np.int16)
        rx.add_channel(kq.channel_config(second_lo=-f, **rcfg))
        tones.append(tone)
        names.append(mode)
    audio = [[] for _ in range(S)]
    status = [[] for _ in range(S)]
    La = Lb // I
    got_all, want_all = [], []
    rng = np.random.default_rng(17)
    for c in range(calls):
        chunk = np.ascontiguousarray(pcm[:, c * per_call * La:(c + 1) * per_call * La])
        cf, s16 = mod.process(chunk, per_call)
        got_all.append(cf)
        want_all.append(model.process(_scaled(chunk), per_call)[0])
        # receiver noise, added on the host (the bank synthesises a noise-free band): 16 LSB rms per component, about
        # 49 dB under each station in a 16 kHz channel.  Without it an FM channel's constant envelope leaves fm.c:101's
        # variance at float rounding, often below zero: snr clips to 0 (fm.c:103), the squelch closes and samples are
        # blanked (fm.c:112-146), as the reference does too.
        noisy = s16.astype(np.float64) + rng.normal(0.0, 16.0, s16.shape)
        rx.push_iq(np.clip(np.round(noisy), -32768, 32767).astype(np.int16))
        assert rx.process() == per_call
        for s in range(S):
            for b in range(per_call):
                audio[s].append(rx.audio(s, b))
                status[s].append(rx.status(s, b))
    mod.close()
    rx.close()
    err = rel_rms(np.concatenate(got_all), np.concatenate(want_all))
    return dict(audio=audio, status=status, tones=tones, names=names, rate=rate, synth_err=err)


# Tone-to-residual bounds (dB, lowest Hz counted), after the first two blocks (2 x 0.82 ms) of 2048 audio samples per
# channel at 39.0625 kHz.  AM counts from 100 Hz: the receiver's AM DC removal is still settling over this short run (the
# audio's block mean falls 39 -> 0.9 over the 64 blocks), and no tone of the test lies below 100 Hz.  Without the added
# noise FM measured 4.1 dB (squelch closed and samples blanked in some blocks, see _loopback).
LOOPBACK_DB = {"usb": (30.0, 0.0), "lsb": (30.0, 0.0), "am": (30.0, 100.0), "fm": (30.0, 0.0)}


def test_loopback_through_the_receiver(gpu):
    """audio in, audio out: the synthesised stream matches the model, every FM channel is open (no squelch, no blanking),
    and every channel's audio after the first two blocks peaks at its tone's bin with the tone 30 dB over the residual"""
    r = _loopback()
    print("loopback: synthesised cf32 vs model, relative RMS %.2e" % r["synth_err"])
    assert r["synth_err"] <= 5e-5
    rows = []
    for s, name in enumerate(r["names"]):
        if name == "fm":
            sts = r["status"][s][2:]
            assert all(x["blanked"] == 0 for x in sts), (s, [x["blanked"] for x in sts])
            assert all(x["squelch_count"] == 0 for x in sts), (s, [x["squelch_count"] for x in sts])
        db_min, lo_hz = LOOPBACK_DB[name]
        rows.append((name,) + _tone_db(np.concatenate(r["audio"][s][2:]), r["rate"], r["tones"][s], lo_hz) + (db_min,))
    for mode in ("am", "usb", "lsb", "fm"):
        m = [x for x in rows if x[0] == mode]
        print("loopback %s: peak-bin error max %d, tone-to-residual min %.1f dB" % (
            mode, max(abs(x[1] - x[2]) for x in m), min(x[3] for x in m)))
    for name, peak, k, db, db_min in rows:
        assert abs(peak - k) <= 1, (name, peak, k)
        assert db >= db_min, (name, db)
