"""Python mirror of the modulator bank (include/ka9q_hip.h: kq_mod_*): modulate.c for many stations at once, summed
into one wideband I/Q stream.  ctypes over libka9q_hip.so; there is no CPU path.
"""
import ctypes as C

import numpy as np

from .bank import Handle, KqError, _err, load_library

KQ_MOD_LINEAR, KQ_MOD_FM = 0, 1
KQ_PCM_F32, KQ_PCM_S16 = 0, 2   # enum kq_pcm_format (KQ_PCM_S16BE = 1 is the AFSK decoder's)

# modulate.c:70-94 (low, high, carrier); FM: the audio band of the FM loopback (+-3000 Hz)
MODES = {
    "am": (KQ_MOD_LINEAR, -5000.0, 5000.0, 1.0),
    "usb": (KQ_MOD_LINEAR, 0.0, 3000.0, 0.0),
    "lsb": (KQ_MOD_LINEAR, -3000.0, 0.0, 0.0),
    "ame": (KQ_MOD_LINEAR, 0.0, 3000.0, 1.0),
    "fm": (KQ_MOD_FM, -3000.0, 3000.0, 0.0),
}


class ModConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("samprate", C.c_int), ("L", C.c_uint), ("M", C.c_uint), ("interp", C.c_uint),
                ("max_stations", C.c_uint), ("max_blocks", C.c_uint), ("stream", C.c_void_p)]


class StationConfig(C.Structure):
    _fields_ = [("mod_type", C.c_int), ("low", C.c_float), ("high", C.c_float), ("carrier", C.c_float),
                ("kaiser_beta", C.c_float), ("deviation", C.c_float), ("frequency", C.c_double), ("sweep", C.c_double),
                ("amplitude_dbfs", C.c_double)]


def station_config(mode="am", frequency=48000.0, amplitude_dbfs=-20.0, sweep=0.0, deviation=3000.0, kaiser_beta=3.0,
                   low=None, high=None, carrier=None):
    """A station with modulate.c's defaults (modulate.c:43-47: 48 kHz, -20 dBFS, no sweep, AM); low / high / carrier
    override the mode's preset."""
    t, lo, hi, car = MODES[mode]
    return StationConfig(t, lo if low is None else low, hi if high is None else high, car if carrier is None else carrier,
                         kaiser_beta, deviation, frequency, sweep, amplitude_dbfs)


def _bind(L):
    if getattr(L, "_kq_mod_bound", False):
        return L
    L.kq_mod_create.restype = C.c_void_p
    L.kq_mod_create.argtypes = [C.POINTER(ModConfig)]
    L.kq_mod_destroy.argtypes = [C.c_void_p]
    L.kq_mod_set_station.argtypes = [C.c_void_p, C.c_uint, C.POINTER(StationConfig)]
    L.kq_mod_remove_station.argtypes = [C.c_void_p, C.c_uint]
    L.kq_mod_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint, C.c_int, C.c_void_p, C.c_void_p]
    L.kq_mod_sync.argtypes = [C.c_void_p]
    L.kq_mod_reset.argtypes = [C.c_void_p]
    L._kq_mod_bound = True
    return L


class ModBank(Handle):
    """Up to max_stations modulate.c stations on one output geometry (Fs, L, M, interp), summed."""
    _destroy = "kq_mod_destroy"

    def __init__(self, samprate, L, M, interp, max_stations, max_blocks, device=0, stream=None):
        self.lib = _bind(load_library())
        cfg = ModConfig(device, samprate, L, M, interp, max_stations, max_blocks, stream)
        self.h = self.lib.kq_mod_create(C.byref(cfg))
        if not self.h:
            raise KqError("kq_mod_create: " + _err(self.lib))
        self.samprate, self.L, self.M, self.interp = samprate, L, M, interp
        self.N = L + M - 1
        self.max_stations, self.max_blocks = max_stations, max_blocks
        self._slots = set()   # occupied slots: the C side reads host rows 0 .. max(self._slots)

    def set_station(self, slot, cfg):
        """add a station to `slot` or change the one there (a StationConfig, e.g. from station_config())"""
        self._chk(self.lib.kq_mod_set_station(self.h, slot, C.byref(cfg)), "kq_mod_set_station")
        self._slots.add(slot)

    def remove_station(self, slot):
        self._chk(self.lib.kq_mod_remove_station(self.h, slot), "kq_mod_remove_station")
        self._slots.discard(slot)

    def process(self, pcm, nblocks, want_cf32=True, want_s16=True):
        """pcm: host float32 or int16 array [rows][>= nblocks * L / interp], row = slot; it must hold rows 0 .. the highest
        occupied slot (rows past it may be left out).  Returns (complex64[nblocks * L] | None, int16[nblocks * L, 2] | None)."""
        pcm = np.asarray(pcm)
        if pcm.dtype == np.int16:
            fmt = KQ_PCM_S16
        else:
            pcm, fmt = np.asarray(pcm, np.float32), KQ_PCM_F32
        pcm = np.ascontiguousarray(pcm)
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        if self._slots and pcm.shape[0] <= max(self._slots):
            raise ValueError("pcm has %d rows; slot %d is occupied" % (pcm.shape[0], max(self._slots)))
        if pcm.shape[1] < nblocks * (self.L // self.interp):
            raise ValueError("pcm rows hold %d samples; %d blocks need %d" % (pcm.shape[1], nblocks, nblocks * (self.L // self.interp)))
        n = nblocks * self.L
        out = np.empty(n, np.complex64) if want_cf32 else None
        s16 = np.empty((n, 2), np.int16) if want_s16 else None
        self._chk(self.lib.kq_mod_process(self.h, pcm.ctypes.data, fmt, pcm.shape[1], nblocks, 0,
                                          out.ctypes.data if want_cf32 else None, s16.ctypes.data if want_s16 else None),
                  "kq_mod_process")
        return out, s16

    def process_device(self, pcm_ptr, pcm_format, stride, nblocks, out_ptr=None, s16_ptr=None):
        """Asynchronous, device pointers (e.g. torch tensors' data_ptr()) on the bank's stream."""
        self._chk(self.lib.kq_mod_process(self.h, pcm_ptr, pcm_format, stride, nblocks, 1, out_ptr, s16_ptr), "kq_mod_process")

    def sync(self):
        self._chk(self.lib.kq_mod_sync(self.h), "kq_mod_sync")

    def reset(self):
        self._chk(self.lib.kq_mod_reset(self.h), "kq_mod_reset")
