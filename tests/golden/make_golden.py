#!/usr/bin/env python3
"""Regenerates tests/golden/*.npz.  Run in the build container (needs /root/reference for the NCO).

  osc_*.npz      : sequences produced by the REFERENCE's own osc.c + dsp.c (oracle/_ref/libref_osc.so):
                   they pin the oracle NCO wherever the tests run.
  decimate_ref.npz : half-band cascades run through the REFERENCE's own decimate.c
                   (oracle/_ref/libref_decimate.so): input, and for three stage mixes the output of two
                   consecutive calls (state carried).
  ref_pins.npz   : what the REFERENCE's own builds (oracle/_ref) answer to the exact inputs of the tests that pin the
                   oracle on them -- test_oracle_osc, test_oracle_decimate, test_oracle_packet -- for boxes where
                   oracle/_ref cannot be built: the full NCO sequences, is_phasor_init, the half-band cascades (two
                   calls, state carried) and crc_good.  Inputs the tests regenerate are pinned by a SHA-256 digest.  The NCO
                   sequences are kept as integer differences of quantised angle and modulus (test_oracle_osc
                   decode_pinned): within 1e-14 of the recorded values, some 35 KB instead of 1.6 MB.
  chain_*.npz    : inputs and outputs of the oracle chain (oracle/libkq_oracle.so).  The reference's
                   filter / demodulator sources need FFTW headers this image lacks, so these are
                   oracle-generated regression vectors, NOT reference outputs (parity unpinned).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import kq_oracle as ko  # noqa: E402
from ka9q_sdr_amd import workload as wl  # noqa: E402
from common import oracle_cfg  # noqa: E402
from test_oracle_osc import PHASOR_INIT_CASES, PIN_BITS, PIN_ERR, SCRIPTS, _run_ref, decode_pinned  # noqa: E402
import test_oracle_decimate as tdec  # noqa: E402
import test_oracle_packet as tpkt  # noqa: E402


def osc():
    assert ko.ref_osc_lib() is not None, "build oracle/_ref first (make -C oracle ref)"
    for name, (script, n) in SCRIPTS.items():
        seq, steps = _run_ref(script, n)
        idx = np.unique(np.concatenate([np.arange(0, n, 97), np.arange(max(0, n - 50), n),
                                        np.arange(16380, min(n, 16390)), np.arange(min(n, 32764), min(n, 32774))]))
        np.savez_compressed(os.path.join(HERE, "osc_%s.npz" % name), index=idx, phasor=seq[idx], steps=steps)


def decimate():
    assert ko.ref_decimate_lib() is not None, "build oracle/_ref first (make -C oracle ref)"
    x = np.random.default_rng(2024).standard_normal(64 << 6).astype(np.float32)
    out = {"x": x}
    for key, (log_dec, thr) in {"l6_t8": (6, 8), "l6_t3": (6, 3), "l4_t0": (4, 0)}.items():
        xs = x[: 64 << log_dec]
        y, st = ko.halfband_cascade(xs, log_dec, thr, use_ref=True)
        y2, _ = ko.halfband_cascade(xs, log_dec, thr, st, use_ref=True)
        out[key] = np.concatenate([y, y2])
        out[key + "_cfg"] = np.array([log_dec, thr])
    np.savez_compressed(os.path.join(HERE, "decimate_ref.npz"), **out)


def encode_pinned(z):
    """[n, 2] phasors -> (second differences of the angle in 2^-PIN_BITS cycle, modulo 2^PIN_BITS and centred; first
    differences of modulus - 1 in 2^-PIN_BITS), both int64; decode_pinned inverts it to within PIN_ERR"""
    one = np.int64(1) << PIN_BITS
    k = np.rint(np.arctan2(z[:, 1], z[:, 0]) / (2 * np.pi) * float(one)).astype(np.int64) & (one - 1)
    d2 = np.diff(k, n=2, prepend=[0, 0]) & (one - 1)
    d2 = np.where(d2 >= one // 2, d2 - one, d2)
    dm = np.diff(np.rint((np.hypot(z[:, 0], z[:, 1]) - 1.0) * float(one)).astype(np.int64), prepend=0)
    err = np.abs(decode_pinned(d2, dm) - z).max()
    assert err < PIN_ERR / 2, err
    return d2, dm


def ref_pins():
    import hashlib
    R = ko.ref_osc_lib()
    assert R is not None and ko.ref_decimate_lib() is not None and ko.ref_ax25_lib() is not None, \
        "build oracle/_ref first (make -C oracle ref)"
    out = {}
    for name, (script, n) in SCRIPTS.items():
        seq, out["osc_%s_steps" % name] = _run_ref(script, n)
        out["osc_%s_d2" % name], out["osc_%s_dm" % name] = encode_pinned(seq)
    out["is_phasor_init"] = np.array([R.is_phasor_init(ko._Cplx(re, im)) for re, im in PHASOR_INIT_CASES])
    for log_dec, thr in tdec.REF_CASES:
        x = tdec._ref_case_input(log_dec, thr)
        b, sb = ko.halfband_cascade(x, log_dec, thr, use_ref=True)
        b2, _ = ko.halfband_cascade(x[::-1].copy(), log_dec, thr, sb, use_ref=True)
        key = "dec_l%d_t%d" % (log_dec, thr)
        out[key], out[key + "_2"] = b, b2
        out[key + "_x_sha256"] = np.array(hashlib.sha256(x.tobytes()).hexdigest())
    A = ko.ref_ax25_lib()
    frames = tpkt._crc_frames()
    out["crc_good"] = np.array([A.crc_good(f, len(f)) for f in frames], np.int32)
    out["crc_frames_sha256"] = np.array(hashlib.sha256(b"".join(frames)).hexdigest())
    np.savez_compressed(os.path.join(HERE, "ref_pins.npz"), **out)


def chain():
    geom = dict(samprate=192000, L=512, M=513, D=4)
    fs, L = geom["samprate"], geom["L"]
    nblocks = 6
    iq = wl.make_iq(fs, nblocks * L, seed=21, emitters=range(24, 40))
    for tag, e, extra in (("fm", 28, {}), ("fmflat", 29, {"flat": 1}), ("am", 30, {}), ("usb", 31, {}), ("lsb", 35, {}),
                          ("isb", 31, {"isb": 1, "channels": 2, "low": -5000.0, "high": 5000.0})):
        p = wl._mode_params(wl.emitter_kind(e), e)
        p.update(second_lo=-(wl.emitter_freq(e, fs) + 2.5))
        p.update(extra)
        cfg = oracle_cfg(p, fs, L, geom["M"], geom["D"], compute_n0=1)
        auds, sts, filts = ko.run_chain(cfg, iq.reshape(nblocks, L), want_filt=True)
        keys = ("if_power", "bb_power", "n0", "snr", "foffset", "pdeviation", "agc_gain", "squelch_count", "hangcount",
                "blanked", "nout")
        np.savez_compressed(os.path.join(HERE, "chain_%s.npz" % tag), iq=iq, audio=np.concatenate(auds),
                            filt=np.concatenate(filts), plan=np.array(repr(p)),
                            **{k: np.array([s[k] for s in sts]) for k in keys})


if __name__ == "__main__":
    decimate()
    osc()
    ref_pins()
    chain()
    print("golden vectors written to", HERE)
