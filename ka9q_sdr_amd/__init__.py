"""ka9q_sdr_amd -- MI355X (gfx950) implementation of ka9q-radio's per-channel DSP hot path.

The compute path is libka9q_hip.so (hand-written HIP kernels behind the C ABI of
include/ka9q_hip.h).  This package is the thin Python mirror of that ABI used by the tests and
by bench.py; there is no CPU or PyTorch fallback: without the built library, or without a GPU,
every compute entry point raises.
"""
from .bank import (  # noqa: F401
    Bank,
    BankConfig,
    ChannelConfig,
    ChanStatus,
    FanoutInfo,
    KQ_AM_DEMOD,
    KQ_FM_DEMOD,
    KQ_FWD_AUTO,
    KQ_FWD_FULL,
    KQ_FWD_PRUNED,
    KQ_IQ_CF32,
    KQ_IQ_S8,
    KQ_IQ_S16,
    KQ_LINEAR_DEMOD,
    KqError,
    build_library,
    channel_config,
    device_count,
    HostBuffer,
    library_path,
    load_library,
)
from .decimate import Decimator  # noqa: F401,E402
from .frontend import FE_STATUS_DTYPE, FrontEnd, KQ_FE_S8, KQ_FE_S16  # noqa: F401,E402
from .packet import AfskBank, KQ_PCM_F32, KQ_PCM_S16BE  # noqa: F401,E402
from . import iqfile  # noqa: F401,E402
from .modulate import KQ_MOD_FM, KQ_MOD_LINEAR, ModBank, StationConfig, station_config  # noqa: F401,E402
from .spectrum import SpecBank, SpecParams, plan, spec_params  # noqa: F401,E402
from .wfm import STATUS_DTYPE, WfmBank, WfmParams, wfm_params  # noqa: F401,E402
from .rds import GROUP_DTYPE, RdsBank, RdsParams, RdsStation, rds_params  # noqa: F401,E402  (rds.STATUS_DTYPE: the rds one)
from .fsk import FskBank, FskParams, fsk_params  # noqa: F401,E402  (fsk.STATUS_DTYPE: the fsk one)
from .ais import ais_nmea, ais_payload_bits, ais_position  # noqa: F401,E402
from .pag import PagBank, PagParams, pag_params  # noqa: F401,E402  (pag.STATUS_DTYPE: the pager one)
from . import pocsag  # noqa: F401,E402
from .tone import ToneBank, ToneParams, tone_params  # noqa: F401,E402  (tone.STATUS_DTYPE: the tone decoder's)
from . import selcall  # noqa: F401,E402
from .cw import CwBank, CwParams, cw_params  # noqa: F401,E402  (cw.STATUS_DTYPE: the Morse decoder's)
from . import morse  # noqa: F401,E402
from .rtty import RttyBank, RttyParams, rtty_params  # noqa: F401,E402  (rtty.STATUS_DTYPE: the RTTY decoder's)
from . import baudot  # noqa: F401,E402
from .psk import PskBank, PskParams, psk_params  # noqa: F401,E402  (psk.STATUS_DTYPE: the PSK decoder's)
from . import varicode  # noqa: F401,E402
from .acars import AcarsBank, AcarsParams, acars_params  # noqa: F401,E402  (acars.STATUS_DTYPE: the ACARS decoder's)
from . import arinc618  # noqa: F401,E402
from .ale import AleBank, AleParams, ale_params  # noqa: F401,E402  (ale.STATUS_DTYPE: the ALE decoder's)
from . import ale2g  # noqa: F401,E402
from .dsc import DscBank, DscParams, dsc_params  # noqa: F401,E402  (dsc.STATUS_DTYPE: the DSC decoder's)
from . import itu493  # noqa: F401,E402
from .navtex import NavtexBank, NavtexParams, navtex_params  # noqa: F401,E402  (navtex.STATUS_DTYPE: the NAVTEX decoder's)
from . import ccir476  # noqa: F401,E402
from .same import SameBank, SameParams, same_params  # noqa: F401,E402  (same.STATUS_DTYPE: the SAME decoder's)
from . import eas  # noqa: F401,E402
from .monitor import KQ_MON_F32, KQ_MON_S16BE, MonBank, MonParams, mon_params  # noqa: F401,E402  (monitor.STATUS_DTYPE: the mixer's)
from .resample import RsmpBank, RsmpParams, rsmp_params  # noqa: F401,E402
