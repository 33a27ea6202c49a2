"""audio-network_amd — MI355X-native acoustic-FSK demodulator (host mirror).

Thin ctypes mirror of the C ABI in include/demod.h (libfskdemod.so built
in-tree from audio-network_amd/csrc). Names, argument meaning and error
behaviour follow the C entry points one-for-one, which in turn mirror the
Opus-decoder-shaped API at the reference's PCM insertion point
(hardware/src/playback.cpp:67-74,115-122).

Every compute call runs the HIP kernels on a gfx950 GPU. There is no CPU
fallback: if libfskdemod.so is missing, :func:`load_library` raises, and if no
MI355X is visible, :class:`Demodulator` raises DemodError(DEMOD_NO_DEVICE).
The frame/packing helpers are host byte work and need no GPU.

Load this package by path (the directory name has a hyphen), e.g.
``importlib.util.spec_from_file_location("audio_network_amd", ".../__init__.py")``.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfskdemod.so")
# FSKD_LIB: another build of the same ABI (measurement A/B of two builds in
# one GPU call, scripts/gpu_run.sh); the product default is the in-tree build
_LIB_ENV = os.environ.get("FSKD_LIB")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "demod.h")

DEMOD_OK = 0
DEMOD_BAD_ARG = -1
DEMOD_BUFFER_TOO_SMALL = -2
DEMOD_INTERNAL_ERROR = -3
DEMOD_INVALID_PACKET = -4
DEMOD_UNIMPLEMENTED = -5
DEMOD_INVALID_STATE = -6
DEMOD_ALLOC_FAIL = -7
DEMOD_DEVICE_ERROR = -8
DEMOD_NO_DEVICE = -9
DEMOD_FRAME_TOO_LARGE = -10

DEMOD_MAX_TONES = 16
DEMOD_OPUS_LOOKAHEAD = 312  # Opus decoder delay at 48 kHz (OpusEncoder.kt:65-67)
DEMOD_MAX_FRAME_PAYLOAD = 4096

CH_LEFT, CH_RIGHT, CH_DOWNMIX = 0, 1, 2
METHOD_AUTO, METHOD_GOERTZEL, METHOD_FFT, METHOD_FOLDED, METHOD_RESIDUE = 0, 1, 2, 3, 4

FSK2_FREQS = (1500.0, 3000.0)                              # SURVEY §8 tone plan
FSK8_FREQS = tuple(1500.0 + 375.0 * i for i in range(8))
BENCH_SEED = 0x2C5DA044


class DemodCfg(ctypes.Structure):
    """Mirror of ``demod_cfg_t`` (include/demod.h)."""
    _fields_ = [
        ("fs", ctypes.c_double),
        ("n", ctypes.c_uint32),
        ("hop", ctypes.c_uint32),
        ("k", ctypes.c_uint32),
        ("channels", ctypes.c_uint32),
        ("channel_mode", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("method", ctypes.c_int32),
        ("lead_in", ctypes.c_uint32),
        ("freqs", ctypes.c_double * DEMOD_MAX_TONES),
    ]


DEMOD_PORT_AUDIO_RX = 58764
DEMOD_PORT_DISCOVERY = 58765
DEMOD_BROADCAST_MAGIC = 0x2C5DA044
DEMOD_INFO_STRING_CAP = 128
DEMOD_MAX_DECODED_FRAME = 11520
DEMOD_MSG_NONE = 0
DEMOD_MSG_DISCOVERY_REQUEST = 2
DEMOD_MSG_DISCOVERY_RESPONSE = 3
DEMOD_MSG_RECEIVER_INFORMATION = 1
DEMOD_MSG_RECEIVER_ERROR = 2


class DemodDiscovery(ctypes.Structure):
    """demod_discovery_t (include/demod.h) = DiscoveryResponse, ip.pb.h:17-24."""
    _fields_ = [
        ("protocol_version", ctypes.c_uint32),
        ("mac_address", ctypes.c_uint64),
        ("device_name", ctypes.c_char * DEMOD_INFO_STRING_CAP),
        ("currently_streaming", ctypes.c_int),
        ("opus_version", ctypes.c_char * DEMOD_INFO_STRING_CAP),
    ]


class DemodReceiverInfo(ctypes.Structure):
    """demod_receiver_info_t = ReceiverInformation, ip.pb.h:55-59."""
    _fields_ = [
        ("discovery_data", DemodDiscovery),
        ("max_encoded_frame_size", ctypes.c_uint32),
        ("max_decoded_frame_size", ctypes.c_uint32),
    ]


class DemodReceiverError(ctypes.Structure):
    """demod_receiver_error_t = ReceiverError, ip.pb.h:26-31."""
    _fields_ = [("audio_underflow", ctypes.c_int), ("audio_decode_error", ctypes.c_int)]


class DemodErrorModel(ctypes.Structure):
    """demod_error_model_t (include/demod.h): the decision rescue's derived bounds."""
    _fields_ = [("method", ctypes.c_int32), ("energy", ctypes.c_int32)] + [
        (f, ctypes.c_double) for f in ("rho_det", "rho_ref", "rho_first", "tau", "tau64", "t2e",
                                        "t2e64", "amb_d")]


class DemodPlanInfo(ctypes.Structure):
    """demod_plan_info_t (include/demod.h): a configuration's tone plan and constants."""
    _fields_ = [
        ("method", ctypes.c_int32), ("log2g", ctypes.c_int32), ("reinsch", ctypes.c_int32),
        ("f16", ctypes.c_int32), ("dcls", ctypes.c_int32), ("slide", ctypes.c_int32),
        ("perm", ctypes.c_uint64),
        ("slot_tone", ctypes.c_int32 * DEMOD_MAX_TONES),
        ("zcls", ctypes.c_int32 * DEMOD_MAX_TONES),
        ("fft_bins", ctypes.c_int32 * DEMOD_MAX_TONES),
        ("coef", ctypes.c_float * DEMOD_MAX_TONES),
        ("sgn", ctypes.c_float * DEMOD_MAX_TONES),
        ("rcoef", ctypes.c_double * DEMOD_MAX_TONES),
        ("rot_len", ctypes.c_uint32),
        ("rot64_len", ctypes.c_uint32),
        ("fold64", ctypes.c_int32),
        ("fft_pmask", ctypes.c_uint32),
    ]


ENERGY_RAW, ENERGY_FOLDED, ENERGY_PARSEVAL = 0, 1, 2

DEMOD_MAX_PHASES = 64
DEMOD_MAX_SYNC = 64
ACQUIRE_TILE = 1024   # DEMOD_ACQUIRE_TILE: windows per workgroup tile of the acquisition scan
DEMOD_MAX_SEGMENTS = 65536


class DemodAcquireResult(ctypes.Structure):
    """demod_acquire_result_t (include/demod.h): phase metric, phase, sync word
    position and the symbol-rate stream's extent."""
    _fields_ = [
        ("metric", ctypes.c_double * DEMOD_MAX_PHASES),
        ("phases", ctypes.c_uint32), ("phase", ctypes.c_uint32),
        ("per_phase", ctypes.c_uint64),
        ("sync_window", ctypes.c_int64),
        ("sync_errors", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("first_window", ctypes.c_uint64), ("n_out", ctypes.c_uint64),
        ("n_written", ctypes.c_uint64),
    ]


def _struct_dict(x: ctypes.Structure) -> dict:
    """The fields of a ctypes structure by name, in the structure's order
    (integers and doubles come out as Python's own)."""
    return {f: getattr(x, f) for f, _ in x._fields_}


def acquire_result_dict(r: "DemodAcquireResult") -> dict:
    """The fields of a DemodAcquireResult; `metric` as float64 [phases]."""
    out = _struct_dict(r)
    out["metric"] = np.array(out.pop("metric")[:r.phases], np.float64)
    return out


class DemodFrameHit(ctypes.Structure):
    """demod_frame_hit_t (include/demod.h): one sync-word hit of a frame scan."""
    _fields_ = [("window", ctypes.c_uint64), ("errors", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DemodFramesResult(ctypes.Structure):
    """demod_frames_result_t (include/demod.h): the phase decision as
    DemodAcquireResult, the hit counts and the incomplete hit at the batch's end."""
    _fields_ = [
        ("metric", ctypes.c_double * DEMOD_MAX_PHASES),
        ("phases", ctypes.c_uint32), ("phase", ctypes.c_uint32),
        ("per_phase", ctypes.c_uint64),
        ("n_hits", ctypes.c_uint64), ("n_written", ctypes.c_uint64),
        ("tail_window", ctypes.c_int64),
        ("tail_errors", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


FRAME_HIT_DTYPE = np.dtype(DemodFrameHit)


def frames_result_dict(r: "DemodFramesResult") -> dict:
    """The fields of a DemodFramesResult; `metric` as float64 [phases]."""
    out = _struct_dict(r)
    out["metric"] = np.array(out.pop("metric")[:r.phases], np.float64)
    return out


DEMOD_CRC16_CCITT_FALSE = 1
DEMOD_CRC32_MPEG2 = 2
DEMOD_CHECK_OK = 0
DEMOD_CHECK_BAD_LENGTH = 1   # len > max_len; crc reported as 0
DEMOD_CHECK_BAD_CRC = 2
CRC_BYTES = {DEMOD_CRC16_CCITT_FALSE: 2, DEMOD_CRC32_MPEG2: 4}


class DemodFrameCheck(ctypes.Structure):
    """demod_frame_check_t (include/demod.h "checked frames"): one row's header
    value, computed CRC, status and covered flag."""
    _fields_ = [("length", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("status", ctypes.c_uint32),
                ("covered", ctypes.c_uint32)]


class DemodFramesCheckResult(ctypes.Structure):
    """demod_frames_check_result_t: a group's rows checked, valid and kept."""
    _fields_ = [("n_checked", ctypes.c_uint64), ("n_valid", ctypes.c_uint64), ("n_kept", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64)]


FRAME_CHECK_DTYPE = np.dtype(DemodFrameCheck)
FRAMES_CHECK_RESULT_DTYPE = np.dtype(DemodFramesCheckResult)


DEMOD_FEC_CONV_K7 = 1          # low nibble: the code. Alone: rate 1/2, coded bits in order
DEMOD_FEC_RATE_2_3 = 0x10
DEMOD_FEC_RATE_3_4 = 0x20      # both rate flags together: refused
DEMOD_FEC_INTERLEAVE = 0x40
DEMOD_FEC_IL_ROWS = 16
DEMOD_FEC_IL_COLS = 16
DEMOD_FEC_DEPTH = 64
FEC_MODES = tuple(DEMOD_FEC_CONV_K7 | r | i for i in (0, DEMOD_FEC_INTERLEAVE)
                  for r in (0, DEMOD_FEC_RATE_2_3, DEMOD_FEC_RATE_3_4))


def fec_row_steps(n_soft: int, fec: int) -> int:
    """St of a row of n_soft = C air soft values in a valid mode (include/
    demod.h "punctured and interleaved"): the greatest T with Nt(T) <= Cu."""
    if fec not in FEC_MODES:
        raise DemodError(DEMOD_BAD_ARG, "fec: not one of the six coded modes")
    cu = int(n_soft) & ~255 if fec & DEMOD_FEC_INTERLEAVE else int(n_soft)
    if fec & DEMOD_FEC_RATE_2_3:
        return 2 * (cu // 3) + (cu % 3 == 2)
    if fec & DEMOD_FEC_RATE_3_4:
        return 3 * (cu // 4) + (0, 0, 1, 2)[cu % 4]
    return cu // 2
DEMOD_DECODE_OK = 0
DEMOD_DECODE_BAD_LENGTH = 1   # len > max_len; metric and steps 0


class DemodFrameDecode(ctypes.Structure):
    """demod_frame_decode_t (include/demod.h "coded frames"): one row's decoded
    length, path metric, status and trellis steps."""
    _fields_ = [("length", ctypes.c_uint32), ("metric", ctypes.c_int32), ("status", ctypes.c_uint32),
                ("steps", ctypes.c_uint32)]


FRAME_DECODE_DTYPE = np.dtype(DemodFrameDecode)


DEMOD_FEC_RS16 = 0x100         # 16 parity bytes a codeword of the outer code, t = 8
DEMOD_FEC_RS32 = 0x200         # 32, t = 16; both parity flags together: refused
DEMOD_RS_OK = 0
DEMOD_RS_BAD_LENGTH = 1        # len > max_len; the other fields 0
DEMOD_RS_FAILED = 2            # at least one codeword failed
RS_PARITY = {0: 0, DEMOD_FEC_RS16: 16, DEMOD_FEC_RS32: 32}
# the 20 modes: none or one of the six coded modes with none or one parity flag; 0 is no mode
RS_MODES = tuple(m | r for r in (0, DEMOD_FEC_RS16, DEMOD_FEC_RS32) for m in (0,) + FEC_MODES if m | r)
RS_PARITY_MODES = tuple(m for m in RS_MODES if m & (DEMOD_FEC_RS16 | DEMOD_FEC_RS32))
RS_CONV_MODES = tuple(m for m in RS_MODES if m & 0xFF)   # with the convolutional code: what the trellis functions take


class DemodFrameRs(ctypes.Structure):
    """demod_frame_rs_t (include/demod.h "Reed-Solomon outer code"): one row's
    status, codewords, corrected bytes and failed codewords."""
    _fields_ = [("status", ctypes.c_uint32), ("codewords", ctypes.c_uint32), ("corrected", ctypes.c_uint32),
                ("failed", ctypes.c_uint32)]


FRAME_RS_DTYPE = np.dtype(DemodFrameRs)


class DemodFrameErase(ctypes.Structure):
    """demod_frame_erase_t (include/demod.h "erasure decoding"): one row's
    flagged bytes, the codewords the first attempt accepted and those that went
    to the errors-only rule."""
    _fields_ = [("erased", ctypes.c_uint32), ("used", ctypes.c_uint32), ("fallback", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


FRAME_ERASE_DTYPE = np.dtype(DemodFrameErase)


def DEMOD_FEC_ERASE(level: int) -> int:
    """The level's field of `fec` (include/demod.h "erasure decoding"): only with
    a parity flag and fec & 0xFF == 0, and only for frames_coded and DemodRx."""
    return (int(level) & 0x7F) << 16


def erase_mode_parts(fec: int) -> Tuple[int, int]:
    """(the mode without the level, the level) of a mode frames_coded and the
    receiver take: one of the 20 modes, with a level only where there is a
    parity flag and no convolutional code."""
    fec = int(fec)
    level, base = (fec >> 16) & 0x7F, fec & ~(0x7F << 16)
    if base not in RS_MODES or (level and (base & 0xFF or base not in RS_PARITY_MODES)):
        raise DemodError(DEMOD_BAD_ARG, "fec: not one of the 20 modes, or a level without a parity flag alone")
    return base, level


MAX_ROW_BYTES = 2 + DEMOD_MAX_FRAME_PAYLOAD + 4 + 19 * 32   # the widest row any mode takes: n' = 4710


def mask_words(row_bytes: int) -> int:
    """Wm: the uint64 words of one row's erasure mask."""
    return (int(row_bytes) + 63) // 64


def rs_mode_parts(fec: int) -> Tuple[int, int]:
    """(the coded mode or 0, P) of one of the 20 modes."""
    if fec not in RS_MODES:
        raise DemodError(DEMOD_BAD_ARG, "fec: not one of the 20 modes")
    return fec & 0xFF, RS_PARITY[fec & (DEMOD_FEC_RS16 | DEMOD_FEC_RS32)]


class DemodRxCfg(ctypes.Structure):
    """demod_rx_cfg_t (include/demod.h "receiver"): the frame format and the
    sizes of a receiver."""
    _fields_ = [("sync", ctypes.c_uint8 * DEMOD_MAX_SYNC), ("sync_len", ctypes.c_uint32),
                ("max_errors", ctypes.c_uint32), ("frame_symbols", ctypes.c_uint32),
                ("len_bytes", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("fec", ctypes.c_uint32),
                ("max_frames", ctypes.c_uint32), ("ring_windows", ctypes.c_uint32)]


class DemodRxFrame(ctypes.Structure):
    """demod_rx_frame_t: one emitted frame of a push."""
    _fields_ = [("stream", ctypes.c_uint32), ("length", ctypes.c_uint32), ("window", ctypes.c_uint64),
                ("body", ctypes.c_uint64), ("errors", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class DemodRxStreamState(ctypes.Structure):
    """demod_rx_stream_state_t: one stream's carry state, device and host."""
    _fields_ = [("base", ctypes.c_uint64), ("hold", ctypes.c_uint64), ("dropped", ctypes.c_uint64),
                ("cut_hits", ctypes.c_uint64), ("fill", ctypes.c_uint32), ("keep", ctypes.c_uint32)]


class DemodRxSummary(ctypes.Structure):
    """demod_rx_summary_t: the totals of one push."""
    _fields_ = [("n_frames", ctypes.c_uint64), ("n_bytes", ctypes.c_uint64), ("n_checked", ctypes.c_uint64),
                ("n_valid", ctypes.c_uint64)]


class DemodRxSizes(ctypes.Structure):
    """demod_rx_sizes_t: what demod_rx_sizes reports."""
    _fields_ = [(f, ctypes.c_uint64) for f in (
        "max_len", "row_bytes", "ring_sym_bytes", "ring_mag_bytes", "scan_work_bytes", "decode_work_bytes",
        "collect_work_bytes", "frames_bytes", "bodies_bytes")]


RX_FRAME_DTYPE = np.dtype(DemodRxFrame)
RX_STATE_DTYPE = np.dtype(DemodRxStreamState)
RX_SUMMARY_DTYPE = np.dtype(DemodRxSummary)


class DemodTxCfg(ctypes.Structure):
    """demod_tx_cfg_t (include/demod.h "transmitter"): the frame format, the
    signal and the sizes of a transmitter."""
    _fields_ = [("sync", ctypes.c_uint8 * DEMOD_MAX_SYNC), ("sync_len", ctypes.c_uint32),
                ("len_bytes", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("fec", ctypes.c_uint32),
                ("max_len", ctypes.c_uint32), ("gap", ctypes.c_uint32),
                ("idle", ctypes.c_uint8 * DEMOD_MAX_SYNC), ("idle_len", ctypes.c_uint32),
                ("amplitude", ctypes.c_int32), ("sigma", ctypes.c_int32), ("ring_symbols", ctypes.c_uint32),
                ("seed", ctypes.c_uint64), ("max_frames", ctypes.c_uint32), ("max_samples", ctypes.c_uint32)]


class DemodTxStreamState(ctypes.Structure):
    """demod_tx_stream_state_t: one stream's queue and phase state, device and host."""
    _fields_ = [("head", ctypes.c_uint64), ("tail", ctypes.c_uint64), ("accepted", ctypes.c_uint64),
                ("refused", ctypes.c_uint64), ("offset", ctypes.c_uint32), ("phase", ctypes.c_uint32)]


class DemodTxPlace(ctypes.Structure):
    """demod_tx_place_t: where a frame of a send went."""
    _fields_ = [("start", ctypes.c_uint64), ("symbols", ctypes.c_uint32), ("status", ctypes.c_uint32)]


class DemodTxSizes(ctypes.Structure):
    """demod_tx_sizes_t: what demod_tx_sizes reports."""
    _fields_ = [(f, ctypes.c_uint64) for f in (
        "max_symbols", "ring_bytes", "state_bytes", "places_bytes", "records_bytes", "bodies_bytes",
        "pcm_bytes", "modulate_work_bytes")]


TX_STATE_DTYPE = np.dtype(DemodTxStreamState)
TX_RECORD_DTYPE = np.dtype([("length", "<u4"), ("body", "<u4")])                         # demod_tx_record_t
TX_PLACE_DTYPE = np.dtype(DemodTxPlace)
DEMOD_TX_OK, DEMOD_TX_BAD_LENGTH, DEMOD_TX_NO_ROOM = 0, 1, 2


class DemodError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = strerror(code) if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


_lib: Optional[ctypes.CDLL] = None

_P = ctypes.c_void_p
_SZ = ctypes.c_size_t


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libfskdemod.so (raises FileNotFoundError if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if _LIB_ENV and path == LIB_PATH:
        path = _LIB_ENV
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not built: run `make -C audio-network_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    try:
        # Bind the HIP runtime once: torch ships its own libamdhip64.so.7; if it
        # is imported after this library, a second runtime would be loaded.
        import torch  # noqa: F401
    except ImportError:
        pass
    if path != LIB_PATH:
        import sys
        print(f"audio_network_amd: FSKD_LIB override active, loading {path} (measurement A/B "
              "only; entry points that build lacks stay unbound)", file=sys.stderr)
    lib = ctypes.CDLL(path)
    sig = {
        "demod_cfg_default": (None, [ctypes.POINTER(DemodCfg)]),
        "demod_create": (_P, [ctypes.POINTER(DemodCfg), ctypes.POINTER(ctypes.c_int)]),
        "demod_destroy": (None, [_P]),
        "demod_reset": (ctypes.c_int, [_P]),
        "demod_pending": (ctypes.c_int, [_P]),
        "demod_slide_windows": (ctypes.c_int, [_P]),
        "demod_method": (ctypes.c_int, [_P]),
        "demod_max_symbols": (ctypes.c_int, [_P, _SZ]),
        "demod_batch_launches": (ctypes.c_int, [_P, _SZ, ctypes.c_int]),
        "demod_rescue_tau": (ctypes.c_double, [_P]),
        "demod_rescue_tau64": (ctypes.c_double, [_P]),
        "demod_error_model": (ctypes.c_int, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodErrorModel)]),
        "demod_plan_info": (ctypes.c_int, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodPlanInfo),
                                           _P, _SZ, _P, _SZ]),
        "demodulate": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ]),
        "demodulate_mags": (ctypes.c_int, [_P, _P, _SZ, _P, _P, _SZ]),
        "demod_batch": (ctypes.c_int, [_P, _P, _SZ, _P, _P]),
        "demod_batch_async": (ctypes.c_int, [_P, _P, _SZ, _P, _P, _P]),
        "demod_batch_spectrum_async": (ctypes.c_int, [_P, _P, _SZ, _P, _P, _P, _P]),
        "demod_acquire_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg)]),
        "demod_acquire_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _P, _SZ,
                                               _P, _P, _P]),
        "demod_acquire": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _P, _SZ,
                                         ctypes.POINTER(DemodAcquireResult)]),
        "demod_acquire_segments_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ, _SZ]),
        "demod_acquire_segments_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _P, _SZ, _P, _SZ,
                                                        ctypes.c_uint32, _P, _SZ, _P, _P, _SZ, _P]),
        "demod_acquire_segments": (ctypes.c_int, [_P, _P, _SZ, _P, _P, _SZ, _P, _SZ, ctypes.c_uint32,
                                                  _P, _SZ, _P]),
        "demod_segments_layout": (ctypes.c_int, [ctypes.POINTER(DemodCfg), _SZ, _P, _P, _P,
                                                 ctypes.POINTER(_SZ)]),
        "demod_frames_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ]),
        "demod_frames_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _SZ, _P, _P,
                                              _P, _SZ, _P, _P, _SZ, _P]),
        "demod_frames": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _SZ, _P, _P, _P, _SZ,
                                        ctypes.POINTER(DemodFramesResult)]),
        "demod_frames_segments_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ, _SZ]),
        "demod_frames_segments_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _P, _SZ, _P, _SZ,
                                                       ctypes.c_uint32, _SZ, _P, _P, _P, _SZ, _P, _P, _SZ,
                                                       _P]),
        "demod_frames_segments": (ctypes.c_int, [_P, _P, _SZ, _P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _SZ,
                                                 _P, _P, _P, _SZ, _P]),
        "demod_crc": (ctypes.c_uint32, [ctypes.c_int, _P, _SZ]),
        "demod_checked_frame_size": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int]),
        "demod_checked_frame_encode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, _P, _SZ]),
        "demod_frames_check_async": (ctypes.c_int, [_P, _P, _P, _P, _SZ, _SZ, _SZ, _SZ, ctypes.c_int,
                                                    ctypes.c_int, _P, _P, _P, _P, _P]),
        "demod_frames_checked": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _SZ, ctypes.c_int,
                                                ctypes.c_int, _P, _P, _P, _SZ,
                                                ctypes.POINTER(DemodFramesResult),
                                                ctypes.POINTER(DemodFramesCheckResult)]),
        "demod_coded_frame_steps": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int]),
        "demod_coded_frame_symbols": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "demod_coded_frame_encode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, _P, _SZ]),
        "demod_coded_row_bytes": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int]),
        "demod_soft_bits": (ctypes.c_int, [_P, ctypes.c_uint32, _P]),
        "demod_coded_frame_decode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, _P, _SZ,
                                                    ctypes.POINTER(DemodFrameDecode)]),
        "demod_frames_decode_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ, _SZ, _SZ]),
        "demod_fec_air_index": (ctypes.c_longlong, [ctypes.c_int, _SZ]),
        "demod_fec_frame_symbols": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int]),
        "demod_fec_frame_encode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _SZ]),
        "demod_fec_row_bytes": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "demod_fec_frame_decode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _SZ,
                                                  ctypes.POINTER(DemodFrameDecode)]),
        "demod_fec_decode_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ, _SZ, _SZ, ctypes.c_int]),
        "demod_frames_decode_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _P, _SZ, _SZ, _SZ, _SZ,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P,
                                                     _SZ, _P]),
        "demod_frames_check_coded_async": (ctypes.c_int, [_P, _P, _P, _P, _SZ, _SZ, _SZ, _SZ, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P]),
        "demod_frames_coded": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ, ctypes.c_uint32, _SZ, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, _P, _P, _P, _SZ,
                                              ctypes.POINTER(DemodFramesResult),
                                              ctypes.POINTER(DemodFramesCheckResult)]),
        "demod_rs_generator": (ctypes.c_int, [ctypes.c_int, _P]),
        "demod_rs_encode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, _P]),
        "demod_rs_frame_size": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "demod_rs_max_len": (ctypes.c_longlong, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
        "demod_rs_frame_encode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _SZ]),
        "demod_rs_frame_decode": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                 ctypes.POINTER(DemodFrameRs)]),
        "demod_frames_rs_async": (ctypes.c_int, [_P, _P, _P, _SZ, _SZ, _SZ, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, _P, _P]),
        "demod_rs_frame_decode_erasures": (ctypes.c_int, [_P, _SZ, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P,
                                                          _P]),
        "demod_soft_erasures": (ctypes.c_int, [_P, _SZ, ctypes.c_int, _P, _SZ]),
        "demod_frames_erasures_async": (ctypes.c_int, [_P, _P, _P, _SZ, _P, _P, _SZ, _SZ, _SZ, _SZ, ctypes.c_int,
                                                       _P, _P]),
        "demod_frames_rs_erasures_async": (ctypes.c_int, [_P, _P, _P, _P, _SZ, _SZ, _SZ, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, _P, _P, _P]),
        "demod_frame_size": (_SZ, [_SZ]),
        "demod_frame_encode": (ctypes.c_int, [_P, _SZ, _P, _SZ]),
        "demod_frame_decode": (ctypes.c_int, [_P, _SZ, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
        "demod_bits_per_symbol": (ctypes.c_int, [ctypes.c_uint32]),
        "demod_pack_symbols": (ctypes.c_int, [_P, _SZ, ctypes.c_int, _P, _SZ]),
        "demod_unpack_symbols": (ctypes.c_int, [_P, _SZ, ctypes.c_int, _P, _SZ]),
        "demod_frame_symbols": (ctypes.c_longlong, [_P, _SZ, ctypes.c_int, _SZ, _P, _SZ]),
        "demod_frame_symbols_size": (ctypes.c_longlong, [_SZ, ctypes.c_int, _SZ]),
        "demod_frame_streams_async": (ctypes.c_longlong, [_P, _SZ, _SZ, ctypes.c_int, _SZ, _P,
                                                          _P]),
        "demod_broadcast_request_encode": (ctypes.c_int, [_P, _SZ]),
        "demod_broadcast_response_encode": (ctypes.c_int, [ctypes.POINTER(DemodDiscovery), _P,
                                                           _SZ]),
        "demod_broadcast_decode": (ctypes.c_int, [_P, _SZ, ctypes.POINTER(ctypes.c_uint32),
                                                  ctypes.POINTER(DemodDiscovery)]),
        "demod_hello_encode": (ctypes.c_int, [ctypes.POINTER(DemodReceiverInfo), _P, _SZ]),
        "demod_receiver_error_encode": (ctypes.c_int, [ctypes.POINTER(DemodReceiverError), _P,
                                                       _SZ]),
        "demod_to_transmitter_decode": (ctypes.c_int, [_P, _SZ, ctypes.POINTER(DemodReceiverInfo),
                                                       ctypes.POINTER(DemodReceiverError),
                                                       ctypes.POINTER(_SZ)]),
        "demod_streams_create": (_P, [ctypes.POINTER(DemodCfg), _SZ, ctypes.POINTER(ctypes.c_int)]),
        "demod_streams_destroy": (None, [_P]),
        "demod_streams_reset": (ctypes.c_int, [_P, _SZ]),
        "demod_streams_pending": (ctypes.c_int, [_P, _SZ]),
        "demod_streams_max_symbols": (ctypes.c_longlong, [_P, _P]),
        "demod_streams_push": (ctypes.c_int, [_P, _P, _P, _P, _P, _SZ, _P]),
        "demod_streams_push_packets": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, _P, _P, _SZ,
                                                      _P]),
        "demod_rx_sizes": (ctypes.c_int, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodRxCfg), _SZ,
                                          ctypes.POINTER(DemodRxSizes)]),
        "demod_rx_advance_async": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _SZ, _P, _P, _SZ, _SZ, _P, _P, _P,
                                                  _P, _P]),
        "demod_rx_collect_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), _SZ]),
        "demod_rx_collect_async": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _SZ, _SZ,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P,
                                                  _SZ, _P]),
        "demod_rx_create": (_P, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodRxCfg), _SZ,
                                 ctypes.POINTER(ctypes.c_int)]),
        "demod_rx_destroy": (None, [_P]),
        "demod_rx_reset": (ctypes.c_int, [_P, _SZ]),
        "demod_rx_state": (ctypes.c_int, [_P, _SZ, ctypes.POINTER(DemodRxStreamState)]),
        "demod_rx_push": (ctypes.c_int, [_P, _P, _P, ctypes.POINTER(_P), ctypes.POINTER(_P),
                                         ctypes.POINTER(DemodRxSummary)]),
        "demod_tx_frame_symbol_count": (ctypes.c_longlong, [ctypes.POINTER(DemodTxCfg), ctypes.c_uint32, _SZ]),
        "demod_tx_frame_symbols": (ctypes.c_longlong, [ctypes.POINTER(DemodTxCfg), ctypes.c_uint32, _P, _SZ,
                                                       _P, _SZ]),
        "demod_tx_sizes": (ctypes.c_int, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodTxCfg), _SZ,
                                          ctypes.POINTER(DemodTxSizes)]),
        "demod_tx_encode_async": (ctypes.c_int, [_P, ctypes.POINTER(DemodTxCfg), _P, _P, _P, _P, _P, _SZ, _SZ,
                                                 _P, _P]),
        "demod_tx_modulate_workspace_size": (_SZ, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodTxCfg), _SZ]),
        "demod_tx_modulate_async": (ctypes.c_int, [_P, ctypes.POINTER(DemodTxCfg), _P, _P, _P, _SZ, _P, _P,
                                                   _SZ, _P]),
        "demod_tx_create": (_P, [ctypes.POINTER(DemodCfg), ctypes.POINTER(DemodTxCfg), _SZ,
                                 ctypes.POINTER(ctypes.c_int)]),
        "demod_tx_destroy": (None, [_P]),
        "demod_tx_reset": (ctypes.c_int, [_P, _SZ]),
        "demod_tx_state": (ctypes.c_int, [_P, _SZ, ctypes.POINTER(DemodTxStreamState)]),
        "demod_tx_device_buffers": (ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(_P)]),
        "demod_tx_send": (ctypes.c_int, [_P, _P, _SZ, _P, _SZ, _P]),
        "demod_tx_pull": (ctypes.c_longlong, [_P, _P, _P]),
        "demod_synth_fsk": (ctypes.c_int, [ctypes.POINTER(DemodCfg), ctypes.c_uint64,
                                           ctypes.c_uint64, _SZ, ctypes.c_int, ctypes.c_int,
                                           _P, _P, _P]),
        "demod_read_ceiling_async": (ctypes.c_int, [_P, _SZ, _P]),
        "demod_group_unique_id": (ctypes.c_int, [_P]),
        "demod_group_shard": (ctypes.c_int, [_SZ, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_SZ),
                                             ctypes.POINTER(_SZ)]),
        "demod_group_block_bytes": (ctypes.c_longlong, [_SZ, ctypes.c_int, _SZ, _SZ, ctypes.c_int]),
        "demod_group_create": (_P, [ctypes.POINTER(DemodCfg), _SZ, ctypes.c_int, ctypes.c_int, _P,
                                    ctypes.POINTER(ctypes.c_int)]),
        "demod_group_create_local": (_P, [ctypes.POINTER(DemodCfg), _SZ, ctypes.c_int, _P,
                                          ctypes.POINTER(ctypes.c_int)]),
        "demod_group_destroy": (None, [_P]),
        "demod_group_world": (ctypes.c_int, [_P]),
        "demod_group_local_ranks": (ctypes.c_int, [_P]),
        "demod_group_rank_shard": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                  ctypes.POINTER(_SZ), ctypes.POINTER(_SZ)]),
        "demod_group_rank_device": (ctypes.c_int, [_P, ctypes.c_int]),
        "demod_group_status": (ctypes.c_int, [_P]),
        "demod_group_wait": (ctypes.c_int, [_P, _P]),
        "demod_group_push": (ctypes.c_int, [_P, _P, _P, _P, _SZ, _P]),
        "demod_group_bucket_async": (ctypes.c_longlong, [_P, _P, _SZ, _SZ, _SZ, _P, _P]),
        "demod_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "demod_version_string": (ctypes.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        if _LIB_ENV and not hasattr(lib, name):
            continue  # an older build for an A/B: entry points it predates stay unbound
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def header_exports(path: str = HEADER_PATH) -> list:
    """Function names declared in include/demod.h."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", src)
    skip = {"defined", "sizeof"}
    decl = []
    for m in re.finditer(r"^[^#\n][^;{}]*?\b([a-z_][a-z0-9_]*)\s*\([^;{}]*\)\s*;", src, flags=re.M):
        if m.group(1) not in skip and not m.group(0).lstrip().startswith("typedef"):
            decl.append(m.group(1))
    return sorted(set(decl)) if decl else sorted(set(names) - skip)


def strerror(code: int) -> str:
    return load_library().demod_strerror(code).decode()


def version_string() -> str:
    return load_library().demod_version_string().decode()


def make_cfg(fs: float = 48000.0, n: int = 1024, hop: Optional[int] = None,
             freqs: Sequence[float] = FSK2_FREQS, channels: int = 1,
             channel_mode: int = CH_LEFT, device: int = 0,
             method: int = METHOD_AUTO, lead_in: int = 0) -> DemodCfg:
    cfg = DemodCfg()
    load_library().demod_cfg_default(ctypes.byref(cfg))
    cfg.fs = float(fs)
    cfg.n = int(n)
    cfg.hop = int(n if hop is None else hop)
    if len(freqs) > DEMOD_MAX_TONES:
        raise DemodError(DEMOD_BAD_ARG, "too many tones")
    cfg.k = len(freqs)
    cfg.channels = int(channels)
    cfg.channel_mode = int(channel_mode)
    cfg.device = int(device)
    cfg.method = int(method)
    cfg.lead_in = int(lead_in)
    for i in range(DEMOD_MAX_TONES):
        cfg.freqs[i] = float(freqs[i]) if i < len(freqs) else 0.0
    return cfg


def error_model(cfg: DemodCfg) -> dict:
    """demod_error_model: the decision rescue's bounds for cfg's tone plan (no GPU)."""
    m = DemodErrorModel()
    rc = load_library().demod_error_model(ctypes.byref(cfg), ctypes.byref(m))
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_error_model")
    return _struct_dict(m)


def plan_info(cfg: DemodCfg) -> dict:
    """demod_plan_info: the plan cfg runs and its fp32 constants (no GPU); `rot`
    as float32 [rot_len][4], `rot64` as float64 (empty without a first pass)."""
    lib = load_library()
    info = DemodPlanInfo()
    rc = lib.demod_plan_info(ctypes.byref(cfg), ctypes.byref(info), None, 0, None, 0)
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_plan_info")
    rot = np.zeros((info.rot_len, 4), np.float32)
    rot64 = np.zeros(info.rot64_len, np.float64)
    rc = lib.demod_plan_info(ctypes.byref(cfg), ctypes.byref(info), _ptr(rot), rot.size,
                             _ptr(rot64), rot64.size)
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_plan_info")
    out = _struct_dict(info)
    for f in ("slot_tone", "zcls", "fft_bins", "coef", "sgn", "rcoef"):
        out[f] = np.array(out[f][:cfg.k])
    out["coef"] = out["coef"].astype(np.float32)
    out["sgn"] = out["sgn"].astype(np.float32)
    out["rot"] = rot
    out["rot64"] = rot64
    return out


def _size(name: str, cfg: DemodCfg, *counts: int, also: tuple = ()) -> int:
    """The size_t the library's function `name` reports for cfg (then `also`:
    further structures by reference) and the counts; a negative count or a
    reported 0 raises DemodError(DEMOD_BAD_ARG, name)."""
    size = 0
    if min(counts, default=0) >= 0:
        size = int(getattr(load_library(), name)(ctypes.byref(cfg), *also, *(int(c) for c in counts)))
    if size == 0:
        raise DemodError(DEMOD_BAD_ARG, name)
    return size


def acquire_workspace_size(cfg: DemodCfg) -> int:
    """demod_acquire_workspace_size: bytes of d_work an acquisition of cfg needs
    (no GPU). Raises DemodError(DEMOD_BAD_ARG) where the configuration has no
    acquisition (n % hop != 0, more than DEMOD_MAX_PHASES phases)."""
    return _size("demod_acquire_workspace_size", cfg)


def acquire_segments_workspace_size(cfg: DemodCfg, max_segments: int, max_windows: int) -> int:
    """demod_acquire_segments_workspace_size: bytes of d_work a segmented
    acquisition of up to max_segments segments over a batch of up to max_windows
    windows needs (no GPU); monotone in both. Raises DemodError(DEMOD_BAD_ARG)
    where it is 0 (no acquisition for cfg, max_segments not in 1 ..
    DEMOD_MAX_SEGMENTS, max_windows >= 2^31)."""
    return _size("demod_acquire_segments_workspace_size", cfg, max_segments, max_windows)


def frames_workspace_size(cfg: DemodCfg, max_windows: int) -> int:
    """demod_frames_workspace_size: bytes of d_work a frame scan of up to
    max_windows windows needs (no GPU); monotone in max_windows. Raises
    DemodError(DEMOD_BAD_ARG) where it is 0 (no acquisition for cfg,
    max_windows >= 2^31)."""
    return _size("demod_frames_workspace_size", cfg, max_windows)


def frames_segments_workspace_size(cfg: DemodCfg, max_segments: int, max_windows: int) -> int:
    """demod_frames_segments_workspace_size: bytes of d_work a segmented frame
    scan of up to max_segments segments over a batch of up to max_windows
    windows needs (no GPU); monotone in both. Raises DemodError(DEMOD_BAD_ARG)
    where it is 0 (no acquisition for cfg, max_segments not in 1 ..
    DEMOD_MAX_SEGMENTS, max_windows >= 2^31)."""
    return _size("demod_frames_segments_workspace_size", cfg, max_segments, max_windows)


def segments_layout(cfg: DemodCfg, n_samples):
    """demod_segments_layout: the batch layout demod_streams_push builds, from
    the runs' lengths in mono samples. Returns (first uint64 [S], count uint32
    [S], n_windows): run s is batch windows first[s] .. first[s] + count[s] - 1
    and starts at sample first[s] * hop of the batch (no GPU)."""
    lens = np.ascontiguousarray(n_samples, dtype=np.uint64).reshape(-1)
    first = np.zeros(lens.size, np.uint64)
    count = np.zeros(lens.size, np.uint32)
    W = _SZ(0)
    rc = load_library().demod_segments_layout(ctypes.byref(cfg), lens.size, _ptr(lens) if lens.size else None,
                                              _ptr(first), _ptr(count), ctypes.byref(W))
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_segments_layout")
    return first, count, int(W.value)


def _sync_bytes(sync) -> np.ndarray:
    return np.zeros(0, np.uint8) if sync is None else np.ascontiguousarray(sync, dtype=np.uint8).reshape(-1)


def frames_decode_workspace_size(cfg: DemodCfg, n_groups: int, max_frames: int, frame_symbols: int) -> int:
    """demod_frames_decode_workspace_size: bytes of d_work a decode of n_groups
    x max_frames rows of frame_symbols symbols needs (no GPU). Raises
    DemodError(DEMOD_BAD_ARG) where it is 0."""
    return _size("demod_frames_decode_workspace_size", cfg, n_groups, max_frames, frame_symbols)


def fec_decode_workspace_size(cfg: DemodCfg, n_groups: int, max_frames: int, frame_symbols: int,
                              fec: int = DEMOD_FEC_CONV_K7) -> int:
    """demod_fec_decode_workspace_size: frames_decode_workspace_size with the
    mode's St (no GPU). Raises DemodError(DEMOD_BAD_ARG) where it is 0."""
    if fec not in RS_CONV_MODES:
        raise DemodError(DEMOD_BAD_ARG, "fec: not one of the six coded modes, with or without a parity flag")
    return _size("demod_fec_decode_workspace_size", cfg, n_groups, max_frames, frame_symbols, fec)


def make_rx_cfg(sync, max_errors: int = 0, frame_symbols: int = 0, len_bytes: int = 2,
                crc: int = DEMOD_CRC16_CCITT_FALSE, fec: int = 0, max_frames: int = 8,
                ring_windows: int = 0) -> DemodRxCfg:
    """A demod_rx_cfg_t (include/demod.h "receiver"). Nothing is judged here:
    rx_sizes and Receiver refuse what the library refuses."""
    word = _sync_bytes(sync)
    if word.size > DEMOD_MAX_SYNC:
        raise DemodError(DEMOD_BAD_ARG, "sync longer than DEMOD_MAX_SYNC")
    x = DemodRxCfg()
    for i, v in enumerate(word.tolist()):
        x.sync[i] = v
    x.sync_len = word.size
    for name, v in (("max_errors", max_errors), ("frame_symbols", frame_symbols), ("len_bytes", len_bytes),
                    ("crc", crc), ("fec", fec), ("max_frames", max_frames), ("ring_windows", ring_windows)):
        if not 0 <= int(v) < 2 ** 32:
            raise DemodError(DEMOD_BAD_ARG, f"{name} not in 0 .. 2^32 - 1")
        setattr(x, name, int(v))
    return x


def rx_sizes(cfg: DemodCfg, rxcfg: DemodRxCfg, n_streams: int) -> dict:
    """demod_rx_sizes: max_len, the row width, the ring bytes and every
    workspace size of a push for n_streams streams (no GPU). Raises
    DemodError(DEMOD_BAD_ARG) for what the library refuses."""
    if n_streams < 0:
        raise DemodError(DEMOD_BAD_ARG, "demod_rx_sizes")
    out = DemodRxSizes()
    rc = load_library().demod_rx_sizes(ctypes.byref(cfg), ctypes.byref(rxcfg), int(n_streams), ctypes.byref(out))
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_rx_sizes")
    return _struct_dict(out)


def make_tx_cfg(sync, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE, fec: int = 0, max_len: int = 0,
                gap: int = 0, idle=(0,), amplitude: int = 8000, sigma: int = 0, seed: int = 0,
                ring_symbols: int = 0, max_frames: int = 1, max_samples: int = 8) -> DemodTxCfg:
    """A demod_tx_cfg_t (include/demod.h "transmitter"). Nothing is judged here:
    demod_tx_sizes does that."""
    sb, ib = _sync_bytes(sync), _sync_bytes(idle)
    if sb.size > DEMOD_MAX_SYNC or ib.size > DEMOD_MAX_SYNC:
        raise DemodError(DEMOD_BAD_ARG, "the word and the idle pattern hold at most DEMOD_MAX_SYNC symbols")
    x = DemodTxCfg()
    for i, v in enumerate(sb.tolist()):
        x.sync[i] = v
    for i, v in enumerate(ib.tolist()):
        x.idle[i] = v
    x.sync_len, x.idle_len = sb.size, ib.size
    x.len_bytes, x.crc, x.fec, x.max_len, x.gap = len_bytes, crc, fec, max_len, gap
    x.amplitude, x.sigma, x.seed = amplitude, sigma, seed
    x.ring_symbols, x.max_frames, x.max_samples = ring_symbols, max_frames, max_samples
    return x


def tx_sizes(cfg: DemodCfg, txcfg: DemodTxCfg, n_streams: int) -> dict:
    """demod_tx_sizes: A(max_len) and every buffer's bytes (no GPU). Raises
    DemodError(DEMOD_BAD_ARG) for a pair or a stream count the transmitter refuses."""
    if n_streams < 0:
        raise DemodError(DEMOD_BAD_ARG, "demod_tx_sizes")
    out = DemodTxSizes()
    rc = load_library().demod_tx_sizes(ctypes.byref(cfg), ctypes.byref(txcfg), int(n_streams), ctypes.byref(out))
    if rc < 0:
        raise DemodError(rc, "demod_tx_sizes")
    return _struct_dict(out)


def tx_modulate_workspace_size(cfg: DemodCfg, txcfg: DemodTxCfg, n_streams: int) -> int:
    """demod_tx_modulate_workspace_size (no GPU). Raises DemodError(DEMOD_BAD_ARG)
    where the C function reports 0."""
    return _size("demod_tx_modulate_workspace_size", cfg, n_streams, also=(ctypes.byref(txcfg),))


def tx_frame_symbol_count(txcfg: DemodTxCfg, k: int, length: int) -> int:
    """demod_tx_frame_symbol_count: A(length), the symbols of a frame on the air."""
    if length < 0 or k < 0:
        raise DemodError(DEMOD_BAD_ARG, "demod_tx_frame_symbol_count")
    rc = int(load_library().demod_tx_frame_symbol_count(ctypes.byref(txcfg), int(k), int(length)))
    if rc < 0:
        raise DemodError(rc, "demod_tx_frame_symbol_count")
    return rc


def tx_frame_symbols(txcfg: DemodTxCfg, k: int, data: bytes) -> np.ndarray:
    """demod_tx_frame_symbols: the word and the payload symbols of one frame
    (uint8 [A(len(data))]), the reference of the transmitter's write launch."""
    data = bytes(data)
    A = tx_frame_symbol_count(txcfg, k, len(data))
    out = np.zeros(A, np.uint8)
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    rc = int(load_library().demod_tx_frame_symbols(ctypes.byref(txcfg), int(k), ctypes.addressof(buf), len(data),
                                                   out.ctypes.data, A))
    if rc < 0:
        raise DemodError(rc, "demod_tx_frame_symbols")
    return out


def rx_collect_workspace_size(cfg: DemodCfg, n_streams: int) -> int:
    """demod_rx_collect_workspace_size (no GPU). Raises DemodError(DEMOD_BAD_ARG)
    where it is 0."""
    return _size("demod_rx_collect_workspace_size", cfg, n_streams)


def _ptr(a) -> int:
    """Address of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return 0
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())


_DTYPE_BYTES = {"int16": 2, "uint8": 1, "float32": 4}


def _check_dev(t, what: str, dtype: str, min_numel: int, device: Optional[int] = None,
               nullable: bool = False) -> None:
    """Validate a device tensor handed to the C ABI as a raw pointer: a short,
    strided, wrong-dtype or wrong-device tensor would otherwise become silent
    out-of-bounds device writes. Raises DemodError(DEMOD_BAD_ARG)."""
    if t is None:
        if nullable or min_numel == 0:
            return
        raise DemodError(DEMOD_BAD_ARG, f"{what}: required")
    if isinstance(t, int):
        raise DemodError(DEMOD_BAD_ARG, f"{what}: pass a device tensor, not a raw address")
    if not hasattr(t, "is_contiguous") or not hasattr(t, "device"):
        raise DemodError(DEMOD_BAD_ARG, f"{what}: expected a torch device tensor")
    if str(t.dtype) != "torch." + dtype:
        raise DemodError(DEMOD_BAD_ARG, f"{what}: dtype {t.dtype}, need torch.{dtype}")
    if not t.is_contiguous():
        raise DemodError(DEMOD_BAD_ARG, f"{what}: not contiguous")
    if t.device.type != "cuda" or (device is not None and t.device.index != device):
        raise DemodError(DEMOD_BAD_ARG, f"{what}: on {t.device}, need cuda:{device}")
    if t.numel() < min_numel:
        raise DemodError(DEMOD_BAD_ARG, f"{what}: {t.numel()} elements, need >= {min_numel}")


class _Handle:
    """The lifetime of a library handle: `_h` of `_lib`, given back once to the
    function `_destroy` names. `_h` may be unset (an __init__ that raised)."""
    _destroy = ""

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _aligned16(flat: np.ndarray) -> np.ndarray:
    """flat (int16, 1-D, contiguous) itself where it starts on a 16-byte
    boundary, else a copy that does."""
    if flat.ctypes.data % 16:
        buf = np.empty(flat.size + 8, dtype=np.int16)
        off = (-buf.ctypes.data % 16) // 2
        buf = buf[off:off + flat.size]
        buf[:] = flat
        return buf
    return flat


def _segment_tables(first, count) -> Tuple[np.ndarray, np.ndarray]:
    """A host segment table as the library reads it: first uint64 [S], count
    uint32 [S], S >= 1."""
    first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.uint32).reshape(-1)
    if first.size != count.size or first.size == 0:
        raise DemodError(DEMOD_BAD_ARG, "first and count: one entry per segment, at least one")
    return first, count


def _rows_shape(n_groups: int, max_frames: int, frame_symbols: int, what: str) -> Tuple[int, int, int]:
    """(S, cap, N) of a scan's S x cap rows of N symbols, refused as the
    library refuses them; `what` names the group count in the message."""
    S, cap, N = int(n_groups), int(max_frames), int(frame_symbols)
    if S < 1 or S > DEMOD_MAX_SEGMENTS or cap < 1 or N < 0 or S * cap >= 2 ** 31:
        raise DemodError(DEMOD_BAD_ARG, f"{what} not in 1 .. DEMOD_MAX_SEGMENTS, max_frames < 1, "
                                        f"frame_symbols < 0 or {what} * max_frames >= 2^31")
    return S, cap, N


class Demodulator(_Handle):
    """One demod_t handle (not thread-safe within a handle, like libopus)."""
    _destroy = "demod_destroy"

    def __init__(self, cfg: Optional[DemodCfg] = None, **kw):
        self._lib = load_library()
        self.cfg = cfg if cfg is not None else make_cfg(**kw)
        err = ctypes.c_int(0)
        h = self._lib.demod_create(ctypes.byref(self.cfg), ctypes.byref(err))
        if not h:
            raise DemodError(err.value, "demod_create")
        self._h = h

    @property
    def k(self) -> int:
        return int(self.cfg.k)

    @property
    def n(self) -> int:
        return int(self.cfg.n)

    @property
    def hop(self) -> int:
        return int(self.cfg.hop)

    def reset(self) -> None:
        rc = self._lib.demod_reset(self._h)
        if rc < 0:
            raise DemodError(rc, "demod_reset")

    @property
    def method(self) -> int:
        """Detector in use: METHOD_GOERTZEL, METHOD_FOLDED, METHOD_RESIDUE or METHOD_FFT."""
        return int(self._lib.demod_method(self._h))

    def pending(self) -> int:
        return int(self._lib.demod_pending(self._h))

    @property
    def slide_windows(self) -> int:
        """Windows per tile of the segment-shared kernel (0: windows alone)."""
        return int(self._lib.demod_slide_windows(self._h))

    def max_symbols(self, n_frames: int) -> int:
        return int(self._lib.demod_max_symbols(self._h, n_frames))

    @property
    def rescue_tau(self) -> float:
        """The decision rescue's threshold factor tau (demod_rescue_tau; 0: off)."""
        return float(self._lib.demod_rescue_tau(self._h))

    @property
    def rescue_tau64(self) -> float:
        """The in-kernel rescue's double-stage threshold factor
        (demod_rescue_tau64; 0: flagged windows take the exact chain)."""
        return float(self._lib.demod_rescue_tau64(self._h))

    def batch_launches(self, n_windows: int, mags: bool = True) -> int:
        """Kernel launches one batch of n_windows makes (demod_batch_launches)."""
        return int(self._lib.demod_batch_launches(self._h, n_windows, 1 if mags else 0))

    def demodulate(self, pcm: np.ndarray, mags: bool = False, max_symbols: Optional[int] = None):
        """Streaming demodulate(pcm, n): pcm is int16, interleaved if stereo."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        ch = int(self.cfg.channels)
        if pcm.size % ch:
            raise DemodError(DEMOD_BAD_ARG, "pcm length not a multiple of channels")
        n_frames = pcm.size // ch
        cap = self.max_symbols(n_frames) if max_symbols is None else int(max_symbols)
        sym = np.empty(max(cap, 1), dtype=np.uint8)
        mag = np.empty((max(cap, 1), self.k), dtype=np.float32) if mags else None
        rc = self._lib.demodulate_mags(self._h, _ptr(pcm), n_frames, _ptr(sym), _ptr(mag), cap)
        if rc < 0:
            raise DemodError(rc, "demodulate")
        return (sym[:rc], mag[:rc]) if mags else sym[:rc]

    def batch(self, pcm, n_windows: Optional[int] = None, mags: bool = False):
        """Batch hot path on host numpy windows [W][n] (or hop-strided)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        flat = pcm.reshape(-1)
        if n_windows is None:
            if pcm.ndim == 2 and self.hop == self.n:
                n_windows = pcm.shape[0]
            else:
                n_windows = 0 if flat.size < self.n else (flat.size - self.n) // self.hop + 1
        if n_windows and (n_windows - 1) * self.hop + self.n > flat.size:
            raise DemodError(DEMOD_BAD_ARG, "pcm shorter than n_windows")
        buf = _aligned16(flat)
        sym = np.empty(max(n_windows, 1), dtype=np.uint8)
        mag = np.empty((max(n_windows, 1), self.k), dtype=np.float32) if mags else None
        rc = self._lib.demod_batch(self._h, _ptr(buf), n_windows, _ptr(sym), _ptr(mag))
        if rc < 0:
            raise DemodError(rc, "demod_batch")
        return (sym[:rc], mag[:rc]) if mags else sym[:rc]

    def _check_batch(self, d_pcm, n_windows: int, d_sym, d_mag, d_spec=None) -> None:
        n_windows = int(n_windows)
        if n_windows < 0:
            raise DemodError(DEMOD_BAD_ARG, "n_windows < 0")
        dev = int(self.cfg.device)
        need = (n_windows - 1) * self.hop + self.n if n_windows else 0
        _check_dev(d_pcm, "d_pcm", "int16", need, dev)
        _check_dev(d_sym, "d_sym", "uint8", n_windows, dev)
        _check_dev(d_mag, "d_mag", "float32", n_windows * self.k, dev, nullable=True)
        _check_dev(d_spec, "d_spec", "float32", n_windows * (self.n // 2 + 1), dev, nullable=True)

    def batch_device(self, d_pcm, n_windows: int, d_sym, d_mag=None) -> int:
        """Synchronous batch on device tensors (checked: dtype, contiguity,
        device, size)."""
        self._check_batch(d_pcm, n_windows, d_sym, d_mag)
        rc = self._lib.demod_batch(self._h, _ptr(d_pcm), n_windows, _ptr(d_sym), _ptr(d_mag))
        if rc < 0:
            raise DemodError(rc, "demod_batch")
        return rc

    def batch_async(self, d_pcm, n_windows: int, d_sym, d_mag=None, stream: int = 0) -> int:
        """Enqueue on a HIP stream (raw hipStream_t as int; 0 = default stream,
        e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check_batch(d_pcm, n_windows, d_sym, d_mag)
        rc = self._lib.demod_batch_async(self._h, _ptr(d_pcm), n_windows, _ptr(d_sym),
                                         _ptr(d_mag), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_batch_async")
        return rc

    def batch_spectrum_async(self, d_pcm, n_windows: int, d_sym, d_mag=None, d_spec=None,
                             stream: int = 0) -> int:
        """FFT handles: symbols, tone-bin |X|^2 and the full |X[b]|^2 spectrum."""
        self._check_batch(d_pcm, n_windows, d_sym, d_mag, d_spec)
        rc = self._lib.demod_batch_spectrum_async(self._h, _ptr(d_pcm), n_windows, _ptr(d_sym),
                                                  _ptr(d_mag), _ptr(d_spec), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_batch_spectrum_async")
        return rc

    def _stage(self, pcm, n_windows: Optional[int] = None):
        """(buf, n_windows) of a call that takes the sliding windows of pcm: a
        host int16 array, flat and copied where it does not start on a 16-byte
        boundary, or a device tensor, checked. n_windows None: all that fit."""
        host = isinstance(pcm, np.ndarray) or not hasattr(pcm, "data_ptr")
        if host:
            flat = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
            size = flat.size
        else:
            size = int(pcm.numel())
        if n_windows is None:
            n_windows = 0 if size < self.n else (size - self.n) // self.hop + 1
        n_windows = int(n_windows)
        need = (n_windows - 1) * self.hop + self.n if n_windows > 0 else 0
        if host:
            if need > size:
                raise DemodError(DEMOD_BAD_ARG, "pcm shorter than n_windows")
            return _aligned16(flat), n_windows
        _check_dev(pcm, "pcm", "int16", need, int(self.cfg.device))
        return pcm, n_windows

    def acquire(self, pcm, n_windows: Optional[int] = None, sync=None, max_errors: int = 0,
                cap: Optional[int] = None):
        """demod_acquire: the detector over the sliding windows of pcm (a host
        int16 array or a device tensor), then symbol timing and the sync word.
        Returns (symbols after the word at the symbol rate, result dict)."""
        buf, n_windows = self._stage(pcm, n_windows)
        sync = _sync_bytes(sync)
        if cap is None:
            cap = n_windows // max(self.n // self.hop, 1) + 1
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
        res = DemodAcquireResult()
        rc = self._lib.demod_acquire(self._h, _ptr(buf), n_windows, _ptr(sync) if sync.size else None,
                                     sync.size, int(max_errors), _ptr(out), int(cap),
                                     ctypes.byref(res))
        if rc < 0:
            raise DemodError(rc, "demod_acquire")
        return out[:rc], acquire_result_dict(res)

    def acquire_async(self, d_sym, d_mag, n_windows: int, sync, max_errors: int, d_out, d_result,
                      d_work, stream: int = 0) -> None:
        """demod_acquire_async on a batch's device outputs: d_out (uint8, its
        numel is cap; None: no output stream), d_result (uint8,
        sizeof(DemodAcquireResult) bytes) and d_work (uint8,
        acquire_workspace_size bytes) are device tensors, checked like the
        batch calls' (dtype, contiguity, device, size)."""
        n_windows = int(n_windows)
        if n_windows < 0:
            raise DemodError(DEMOD_BAD_ARG, "n_windows < 0")
        dev = int(self.cfg.device)
        _check_dev(d_sym, "d_sym", "uint8", max(n_windows, 1), dev)
        _check_dev(d_mag, "d_mag", "float32", max(n_windows, 1) * self.k, dev)
        _check_dev(d_out, "d_out", "uint8", 0, dev, nullable=True)
        _check_dev(d_result, "d_result", "uint8", ctypes.sizeof(DemodAcquireResult), dev)
        _check_dev(d_work, "d_work", "uint8", acquire_workspace_size(self.cfg), dev)
        sync = _sync_bytes(sync)
        cap = 0 if d_out is None else int(d_out.numel())
        rc = self._lib.demod_acquire_async(self._h, _ptr(d_sym), _ptr(d_mag), n_windows,
                                           _ptr(sync) if sync.size else None, sync.size,
                                           int(max_errors), _ptr(d_out) if cap else None, cap,
                                           _ptr(d_result), _ptr(d_work), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_acquire_async")

    def acquire_segments(self, pcm, first, count, sync=None, max_errors: int = 0,
                         cap: Optional[int] = None, n_windows: Optional[int] = None):
        """demod_acquire_segments: the detector over the sliding windows of pcm
        (a host int16 array or a device tensor), then the acquisition of each
        segment first[s] .. first[s] + count[s] - 1 as a batch of its own.
        Returns (out uint8 [S][cap], row s valid up to its n_written and 0xFF
        after it; [result dict per segment])."""
        buf, n_windows = self._stage(pcm, n_windows)
        first, count = _segment_tables(first, count)
        S = first.size
        sync = _sync_bytes(sync)
        if cap is None:
            cap = int(count.max()) // max(self.n // self.hop, 1) + 1
        cap = int(cap)
        out = np.full((S, max(cap, 1)), 0xFF, dtype=np.uint8)[:, :cap]
        results = (DemodAcquireResult * S)()
        rc = self._lib.demod_acquire_segments(self._h, _ptr(buf), n_windows, _ptr(first), _ptr(count), S,
                                              _ptr(sync) if sync.size else None, sync.size,
                                              int(max_errors), out.ctypes.data if cap else None, cap,
                                              ctypes.cast(results, _P))
        if rc < 0:
            raise DemodError(rc, "demod_acquire_segments")
        return out, [acquire_result_dict(r) for r in results]

    def acquire_segments_async(self, d_sym, d_mag, n_windows: int, d_first, d_count, n_segments: int,
                               sync, max_errors: int, d_out, d_results, d_work,
                               stream: int = 0) -> None:
        """demod_acquire_segments_async on a batch's device outputs. d_first
        (int64 tensor holding the uint64 table) and d_count (int32 tensor
        holding the uint32 table) have n_segments entries; d_out (uint8,
        n_segments * cap bytes: cap is its numel // n_segments; None: no rows),
        d_results (uint8, n_segments * sizeof(DemodAcquireResult) bytes) and
        d_work (uint8, at least acquire_segments_workspace_size(cfg,
        n_segments, n_windows) bytes; all of it is handed over, a larger one
        raises the tile budget) are device tensors, checked like the batch
        calls' (dtype, contiguity, device, size)."""
        n_windows, S = int(n_windows), int(n_segments)
        if n_windows < 0 or S < 1 or S > DEMOD_MAX_SEGMENTS:
            raise DemodError(DEMOD_BAD_ARG, "n_windows < 0 or n_segments not in 1 .. DEMOD_MAX_SEGMENTS")
        dev = int(self.cfg.device)
        _check_dev(d_sym, "d_sym", "uint8", max(n_windows, 1), dev)
        _check_dev(d_mag, "d_mag", "float32", max(n_windows, 1) * self.k, dev)
        _check_dev(d_first, "d_first", "int64", S, dev)
        _check_dev(d_count, "d_count", "int32", S, dev)
        _check_dev(d_out, "d_out", "uint8", 0, dev, nullable=True)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodAcquireResult), dev)
        _check_dev(d_work, "d_work", "uint8",
                   acquire_segments_workspace_size(self.cfg, S, n_windows), dev)
        sync = _sync_bytes(sync)
        cap = 0 if d_out is None else int(d_out.numel()) // S
        rc = self._lib.demod_acquire_segments_async(
            self._h, _ptr(d_sym), _ptr(d_mag), n_windows, _ptr(d_first), _ptr(d_count), S,
            _ptr(sync) if sync.size else None, sync.size, int(max_errors),
            _ptr(d_out) if cap else None, cap, _ptr(d_results), _ptr(d_work), int(d_work.numel()),
            stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_acquire_segments_async")

    def frames(self, pcm, sync, max_errors: int = 0, frame_symbols: int = 0,
               max_frames: Optional[int] = None, n_windows: Optional[int] = None,
               payload: bool = True, packed: bool = True):
        """demod_frames: the detector over the sliding windows of pcm (a host
        int16 array or a device tensor), then every sync-word hit on the
        acquired phase with its frame_symbols payload symbols. Returns (hits: a
        FRAME_HIT_DTYPE array [n_written], payload uint8 [n_written][N] or None,
        packed uint8 [n_written][ceil(N bits / 8)] or None, result dict).
        Overlapping hits are all listed (include/demod.h "frame scan")."""
        buf, n_windows = self._stage(pcm, n_windows)
        sync = _sync_bytes(sync)
        N = int(frame_symbols)
        if N < 0 or (max_frames is not None and max_frames < 0):
            raise DemodError(DEMOD_BAD_ARG, "frame_symbols or max_frames < 0")
        if max_frames is None:
            max_frames = n_windows // max(self.n // self.hop, 1) + 1
        cap = int(max_frames)
        B = (N * bits_per_symbol(self.k) + 7) // 8
        hits = np.zeros(max(cap, 1), dtype=FRAME_HIT_DTYPE)
        pay = np.empty((max(cap, 1), N), dtype=np.uint8) if payload and N else None
        pak = np.empty((max(cap, 1), B), dtype=np.uint8) if packed and N else None
        res = DemodFramesResult()
        rc = self._lib.demod_frames(self._h, _ptr(buf), n_windows, _ptr(sync) if sync.size else None,
                                    sync.size, int(max_errors), N, _ptr(hits) if cap else None,
                                    _ptr(pay) if pay is not None else None,
                                    _ptr(pak) if pak is not None else None, cap, ctypes.byref(res))
        if rc < 0:
            raise DemodError(rc, "demod_frames")
        return (hits[:rc], pay[:rc] if pay is not None else None,
                pak[:rc] if pak is not None else None, frames_result_dict(res))

    def frames_async(self, d_sym, d_mag, n_windows: int, sync, max_errors: int, frame_symbols: int,
                     d_hits, d_payload, d_packed, max_frames: int, d_result, d_work,
                     stream: int = 0) -> None:
        """demod_frames_async on a batch's device outputs. d_hits (uint8,
        max_frames * sizeof(DemodFrameHit) bytes; None with max_frames 0),
        d_payload (uint8, max_frames * frame_symbols bytes, or None), d_packed
        (uint8, max_frames * ceil(frame_symbols * bits / 8) bytes, or None),
        d_result (uint8, sizeof(DemodFramesResult) bytes) and d_work (uint8, at
        least frames_workspace_size(cfg, n_windows) bytes) are device tensors,
        checked like the batch calls' (dtype, contiguity, device, size)."""
        n_windows, N, cap = int(n_windows), int(frame_symbols), int(max_frames)
        if n_windows < 0 or N < 0 or cap < 0:
            raise DemodError(DEMOD_BAD_ARG, "n_windows, frame_symbols or max_frames < 0")
        dev = int(self.cfg.device)
        B = (N * bits_per_symbol(self.k) + 7) // 8
        _check_dev(d_sym, "d_sym", "uint8", max(n_windows, 1), dev)
        _check_dev(d_mag, "d_mag", "float32", max(n_windows, 1) * self.k, dev)
        _check_dev(d_hits, "d_hits", "uint8", cap * ctypes.sizeof(DemodFrameHit), dev)
        _check_dev(d_payload, "d_payload", "uint8", cap * N, dev, nullable=True)
        _check_dev(d_packed, "d_packed", "uint8", cap * B, dev, nullable=True)
        _check_dev(d_result, "d_result", "uint8", ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_work, "d_work", "uint8", frames_workspace_size(self.cfg, n_windows), dev)
        sync = _sync_bytes(sync)
        rc = self._lib.demod_frames_async(
            self._h, _ptr(d_sym), _ptr(d_mag), n_windows, _ptr(sync) if sync.size else None, sync.size,
            int(max_errors), N, _ptr(d_hits) if d_hits is not None else None,
            _ptr(d_payload) if d_payload is not None else None,
            _ptr(d_packed) if d_packed is not None else None, cap, _ptr(d_result), _ptr(d_work),
            int(d_work.numel()), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_async")

    def frames_segments(self, pcm, first, count, sync, max_errors: int = 0, frame_symbols: int = 0,
                        max_frames: Optional[int] = None, n_windows: Optional[int] = None,
                        payload: bool = True, packed: bool = True):
        """demod_frames_segments: the detector over the sliding windows of pcm
        (a host int16 array or a device tensor), then the frame scan of each
        segment first[s] .. first[s] + count[s] - 1 as a batch of its own.
        Returns one (hits FRAME_HIT_DTYPE [n_written], payload uint8
        [n_written][N] or None, packed uint8 [n_written][ceil(N bits / 8)] or
        None, result dict) per segment; a hit's window is relative to its
        segment's first window."""
        buf, n_windows = self._stage(pcm, n_windows)
        first, count = _segment_tables(first, count)
        S = first.size
        sync = _sync_bytes(sync)
        N = int(frame_symbols)
        if N < 0 or (max_frames is not None and max_frames < 0):
            raise DemodError(DEMOD_BAD_ARG, "frame_symbols or max_frames < 0")
        if max_frames is None:
            max_frames = int(count.max()) // max(self.n // self.hop, 1) + 1
        cap = int(max_frames)
        B = (N * bits_per_symbol(self.k) + 7) // 8
        hits = np.zeros((S, max(cap, 1)), dtype=FRAME_HIT_DTYPE)
        pay = np.empty((S, max(cap, 1), N), dtype=np.uint8) if payload and N else None
        pak = np.empty((S, max(cap, 1), B), dtype=np.uint8) if packed and N else None
        results = (DemodFramesResult * S)()
        rc = self._lib.demod_frames_segments(
            self._h, _ptr(buf), n_windows, _ptr(first), _ptr(count), S, _ptr(sync) if sync.size else None,
            sync.size, int(max_errors), N, _ptr(hits) if cap else None,
            _ptr(pay) if pay is not None else None, _ptr(pak) if pak is not None else None, cap,
            ctypes.cast(results, _P))
        if rc < 0:
            raise DemodError(rc, "demod_frames_segments")
        out = []
        for s, r in enumerate(results):
            nw = int(r.n_written)
            out.append((hits[s, :nw].copy(), pay[s, :nw].copy() if pay is not None else None,
                        pak[s, :nw].copy() if pak is not None else None, frames_result_dict(r)))
        return out

    def frames_segments_async(self, d_sym, d_mag, n_windows: int, d_first, d_count, n_segments: int,
                              sync, max_errors: int, frame_symbols: int, d_hits, d_payload, d_packed,
                              max_frames: int, d_results, d_work, stream: int = 0) -> None:
        """demod_frames_segments_async on a batch's device outputs. d_first
        (int64 tensor holding the uint64 table) and d_count (int32 tensor
        holding the uint32 table) have n_segments entries; d_hits (uint8,
        n_segments * max_frames * sizeof(DemodFrameHit) bytes; None with
        max_frames 0), d_payload (uint8, n_segments * max_frames *
        frame_symbols bytes, or None), d_packed (uint8, n_segments * max_frames
        * ceil(frame_symbols * bits / 8) bytes, or None), d_results (uint8,
        n_segments * sizeof(DemodFramesResult) bytes) and d_work (uint8, at
        least frames_segments_workspace_size(cfg, n_segments, n_windows) bytes;
        all of it is handed over, a larger one raises the tile budget) are
        device tensors, checked like the batch calls' (dtype, contiguity,
        device, size)."""
        n_windows, S, N, cap = int(n_windows), int(n_segments), int(frame_symbols), int(max_frames)
        if n_windows < 0 or N < 0 or cap < 0 or S < 1 or S > DEMOD_MAX_SEGMENTS:
            raise DemodError(DEMOD_BAD_ARG, "n_windows, frame_symbols or max_frames < 0, or n_segments "
                                            "not in 1 .. DEMOD_MAX_SEGMENTS")
        dev = int(self.cfg.device)
        B = (N * bits_per_symbol(self.k) + 7) // 8
        _check_dev(d_sym, "d_sym", "uint8", max(n_windows, 1), dev)
        _check_dev(d_mag, "d_mag", "float32", max(n_windows, 1) * self.k, dev)
        _check_dev(d_first, "d_first", "int64", S, dev)
        _check_dev(d_count, "d_count", "int32", S, dev)
        _check_dev(d_hits, "d_hits", "uint8", S * cap * ctypes.sizeof(DemodFrameHit), dev)
        _check_dev(d_payload, "d_payload", "uint8", S * cap * N, dev, nullable=True)
        _check_dev(d_packed, "d_packed", "uint8", S * cap * B, dev, nullable=True)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_work, "d_work", "uint8", frames_segments_workspace_size(self.cfg, S, n_windows), dev)
        sync = _sync_bytes(sync)
        rc = self._lib.demod_frames_segments_async(
            self._h, _ptr(d_sym), _ptr(d_mag), n_windows, _ptr(d_first), _ptr(d_count), S,
            _ptr(sync) if sync.size else None, sync.size, int(max_errors), N,
            _ptr(d_hits) if d_hits is not None else None,
            _ptr(d_payload) if d_payload is not None else None,
            _ptr(d_packed) if d_packed is not None else None, cap, _ptr(d_results), _ptr(d_work),
            int(d_work.numel()), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_segments_async")

    def _frame_shape(self, frame_symbols: int, len_bytes: int, crc: int, fec: int) -> Tuple[int, int]:
        """(row bytes, max_len) of rows of frame_symbols symbols: B of a checked
        frame's packed rows (fec 0), Bd of a coded frame's decoded rows
        (a coded mode, of its St trellis steps)."""
        if len_bytes not in (1, 2) or crc not in CRC_BYTES:
            raise DemodError(DEMOD_BAD_ARG, "len_bytes not 1 or 2, or an unknown crc kind")
        bits = bits_per_symbol(self.k)
        fec, parity = rs_mode_parts(fec) if fec else (0, 0)
        if fec:
            if self.k != 1 << bits:
                raise DemodError(DEMOD_BAD_ARG, "coded frames need K = 2^bits tones")
            St = fec_row_steps(int(frame_symbols) * bits, fec)
            if St < 8 * len_bytes + DEMOD_FEC_DEPTH:
                raise DemodError(DEMOD_BAD_ARG, "rows shorter than the header look-ahead")
            B, short = (St - 6) // 8, ""
        else:
            B, short = (int(frame_symbols) * bits + 7) // 8, "rows too short for header and CRC, or "
        if parity:
            max_len = rs_max_len(B, len_bytes, crc, DEMOD_FEC_RS16 if parity == 16 else DEMOD_FEC_RS32) \
                if 0 <= B < 2 ** 31 else -1
        else:
            max_len = B - len_bytes - CRC_BYTES[crc]
        if max_len < 0 or max_len > DEMOD_MAX_FRAME_PAYLOAD:
            raise DemodError(DEMOD_BAD_ARG, short + "max_len above DEMOD_MAX_FRAME_PAYLOAD")
        return B, max_len

    def _check_scan_outputs(self, S: int, cap: int, max_len: int, d_hits, d_results, d_check, d_kept, d_body,
                            d_summary, rows: Optional[tuple] = None, collect: bool = False) -> None:
        """The device tensors of a scan of S x cap rows and of its check, in
        the callers' argument order. rows: (tensor, its name, bytes a row) of
        the rows a check reads, between d_hits and d_results. collect: the
        collect step's view, d_body required and the check's summary named
        d_check_summary."""
        dev = int(self.cfg.device)
        n = S * cap
        _check_dev(d_hits, "d_hits", "uint8", n * ctypes.sizeof(DemodFrameHit), dev)
        if rows is not None:
            _check_dev(rows[0], rows[1], "uint8", n * rows[2], dev)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_check, "d_check", "uint8", n * ctypes.sizeof(DemodFrameCheck), dev)
        _check_dev(d_kept, "d_kept", "int32", n, dev)
        _check_dev(d_body, "d_body", "uint8", n * max_len, dev, nullable=not collect)
        _check_dev(d_summary, "d_check_summary" if collect else "d_summary", "uint8",
                   S * ctypes.sizeof(DemodFramesCheckResult), dev)

    def frames_check_async(self, d_hits, d_packed, d_results, n_groups: int, max_frames: int,
                           sync_len: int, frame_symbols: int, len_bytes: int, crc: int, d_check, d_kept,
                           d_body, d_summary, stream: int = 0) -> None:
        """demod_frames_check_async on a frame scan's device outputs (n_groups =
        1 after frames_async, = n_segments after frames_segments_async). d_hits
        (uint8, n_groups * max_frames * sizeof(DemodFrameHit) bytes), d_packed
        (uint8, n_groups * max_frames * B bytes) and d_results (uint8, n_groups
        * sizeof(DemodFramesResult) bytes) are the scan's; d_check (uint8, 16
        bytes a row), d_kept (int32, one a row), d_body (uint8, n_groups *
        max_frames * max_len bytes, or None) and d_summary (uint8, n_groups *
        sizeof(DemodFramesCheckResult) bytes) are written. Device tensors,
        checked like the batch calls' (dtype, contiguity, device, size)."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        B, max_len = self._frame_shape(N, len_bytes, crc, 0)
        self._check_scan_outputs(S, cap, max_len, d_hits, d_results, d_check, d_kept, d_body, d_summary,
                                 rows=(d_packed, "d_packed", B))
        rc = self._lib.demod_frames_check_async(
            self._h, _ptr(d_hits), _ptr(d_packed), _ptr(d_results), S, cap, int(sync_len), N, int(len_bytes),
            int(crc), _ptr(d_check), _ptr(d_kept), _ptr(d_body) if d_body is not None else None,
            _ptr(d_summary), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_check_async")

    def frames_decode_async(self, d_hits, d_mag, n_windows: int, d_first, d_results, n_groups: int,
                            max_frames: int, sync_len: int, frame_symbols: int, len_bytes: int, crc: int,
                            d_rows, d_decode, d_work, fec: int = DEMOD_FEC_CONV_K7, stream: int = 0) -> None:
        """demod_frames_decode_async on a frame scan's device outputs (n_groups =
        1 and d_first None after frames_async; n_groups = n_segments and the
        scan's d_first, an int64 tensor holding the uint64 table, after
        frames_segments_async). d_hits and d_results are the scan's, d_mag
        (float32, n_windows * k) the detector's; d_rows (uint8, n_groups *
        max_frames * Bd bytes) and d_decode (uint8, 16 bytes a row) are
        written; d_work (uint8, at least fec_decode_workspace_size bytes of
        the mode `fec`) may hold anything. Device tensors, checked like the batch calls'."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        W, L = int(n_windows), int(sync_len)
        if W < 0 or W >= 2 ** 31:
            raise DemodError(DEMOD_BAD_ARG, "n_windows not in 0 .. 2^31 - 1")
        if fec not in RS_MODES or not fec & 0xFF:
            raise DemodError(DEMOD_BAD_ARG, "fec: not one of the six coded modes, with or without a parity flag")
        Bd, _ = self._frame_shape(N, len_bytes, crc, fec)
        dev = int(self.cfg.device)
        rows = S * cap
        _check_dev(d_hits, "d_hits", "uint8", rows * ctypes.sizeof(DemodFrameHit), dev)
        _check_dev(d_mag, "d_mag", "float32", max(W, 1) * self.k, dev)
        _check_dev(d_first, "d_first", "int64", S, dev, nullable=True)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_rows, "d_rows", "uint8", rows * Bd, dev)
        _check_dev(d_decode, "d_decode", "uint8", rows * ctypes.sizeof(DemodFrameDecode), dev)
        _check_dev(d_work, "d_work", "uint8", fec_decode_workspace_size(self.cfg, S, cap, N, fec), dev)
        rc = self._lib.demod_frames_decode_async(
            self._h, _ptr(d_hits), _ptr(d_mag), W, _ptr(d_first) if d_first is not None else None,
            _ptr(d_results), S, cap, L, N, int(len_bytes), int(crc), int(fec), _ptr(d_rows), _ptr(d_decode),
            _ptr(d_work), int(d_work.numel()), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_decode_async")

    def frames_check_coded_async(self, d_hits, d_rows, d_results, n_groups: int, max_frames: int,
                                 sync_len: int, frame_symbols: int, len_bytes: int, crc: int, d_check, d_kept,
                                 d_body, d_summary, fec: int = DEMOD_FEC_CONV_K7, stream: int = 0) -> None:
        """demod_frames_check_coded_async: frames_check_async over the rows
        frames_decode_async wrote (uint8, n_groups * max_frames * Bd bytes),
        with max_len = Bd - len_bytes - the CRC's bytes and the coded span."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        if fec not in RS_MODES:
            raise DemodError(DEMOD_BAD_ARG, "fec: not one of the 20 modes")
        Bd, max_len = self._frame_shape(N, len_bytes, crc, fec)
        self._check_scan_outputs(S, cap, max_len, d_hits, d_results, d_check, d_kept, d_body, d_summary,
                                 rows=(d_rows, "d_rows", Bd))
        rc = self._lib.demod_frames_check_coded_async(
            self._h, _ptr(d_hits), _ptr(d_rows), _ptr(d_results), S, cap, int(sync_len), N, int(len_bytes),
            int(crc), int(fec), _ptr(d_check), _ptr(d_kept), _ptr(d_body) if d_body is not None else None,
            _ptr(d_summary), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_check_coded_async")

    def frames_rs_async(self, d_rows, d_results, n_groups: int, max_frames: int, frame_symbols: int,
                        len_bytes: int, crc: int, fec: int, d_rs, stream: int = 0) -> None:
        """demod_frames_rs_async: the Reed-Solomon outer code over the rows of
        a frame scan (fec & 0xFF == 0: its d_packed, B bytes a row) or of
        frames_decode_async (Bd bytes a row), corrected in place before
        frames_check_coded_async reads them. d_rs (uint8, 16 bytes a row:
        FRAME_RS_DTYPE) is written. Device tensors, checked like the batch
        calls'."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        if fec not in RS_PARITY_MODES:
            raise DemodError(DEMOD_BAD_ARG, "fec: not one of the modes with a parity flag")
        W, _ = self._frame_shape(N, len_bytes, crc, fec)
        dev = int(self.cfg.device)
        _check_dev(d_rows, "d_rows", "uint8", S * cap * W, dev)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_rs, "d_rs", "uint8", S * cap * ctypes.sizeof(DemodFrameRs), dev)
        rc = self._lib.demod_frames_rs_async(self._h, _ptr(d_rows), _ptr(d_results), S, cap, N, int(len_bytes),
                                             int(crc), int(fec), _ptr(d_rs), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_rs_async")

    def frames_erasures_async(self, d_hits, d_mag, n_windows: int, d_first, d_results, n_groups: int,
                              max_frames: int, sync_len: int, frame_symbols: int, level: int, d_erase,
                              stream: int = 0) -> None:
        """demod_frames_erasures_async: the erasure masks of the plain rows a
        frame scan listed, from the detector's powers (arguments as
        frames_decode_async's). d_erase (int64 holding the uint64 words,
        n_groups * max_frames * Wm of the packed row's B bytes) is written.
        Device tensors, checked like the batch calls'."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        W = int(n_windows)
        if W < 0 or W >= 2 ** 31:
            raise DemodError(DEMOD_BAD_ARG, "n_windows not in 0 .. 2^31 - 1")
        if not 1 <= int(level) <= 127:
            raise DemodError(DEMOD_BAD_ARG, "level not in 1 .. 127")
        if self.k not in (2, 4, 8, 16):
            raise DemodError(DEMOD_BAD_ARG, "the erasure masks need K = 2, 4, 8 or 16 tones")
        B = (N * bits_per_symbol(self.k) + 7) // 8     # plain rows, whatever header, CRC and parity they are read with
        if not 1 <= B <= MAX_ROW_BYTES:
            raise DemodError(DEMOD_BAD_ARG, "frame_symbols: no row, or one wider than any mode takes")
        dev = int(self.cfg.device)
        _check_dev(d_hits, "d_hits", "uint8", S * cap * ctypes.sizeof(DemodFrameHit), dev)
        _check_dev(d_mag, "d_mag", "float32", max(W, 1) * self.k, dev)
        _check_dev(d_first, "d_first", "int64", S, dev, nullable=True)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_erase, "d_erase", "int64", S * cap * mask_words(B), dev)
        rc = self._lib.demod_frames_erasures_async(
            self._h, _ptr(d_hits), _ptr(d_mag), W, _ptr(d_first) if d_first is not None else None,
            _ptr(d_results), S, cap, int(sync_len), N, int(level), _ptr(d_erase), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_erasures_async")

    def frames_rs_erasures_async(self, d_rows, d_erase, d_results, n_groups: int, max_frames: int,
                                 frame_symbols: int, len_bytes: int, crc: int, fec: int, d_rs, d_erec,
                                 stream: int = 0) -> None:
        """demod_frames_rs_erasures_async: frames_rs_async with the rows'
        erasure masks d_erase (int64 holding the uint64 words, Wm of the row
        width a row); d_erec (uint8, 16 bytes a row: FRAME_ERASE_DTYPE) is
        written beside d_rs."""
        S, cap, N = _rows_shape(n_groups, max_frames, frame_symbols, "n_groups")
        if fec not in RS_PARITY_MODES:
            raise DemodError(DEMOD_BAD_ARG, "fec: not one of the modes with a parity flag")
        W, _ = self._frame_shape(N, len_bytes, crc, fec)
        dev = int(self.cfg.device)
        _check_dev(d_rows, "d_rows", "uint8", S * cap * W, dev)
        _check_dev(d_erase, "d_erase", "int64", S * cap * mask_words(W), dev)
        _check_dev(d_results, "d_results", "uint8", S * ctypes.sizeof(DemodFramesResult), dev)
        _check_dev(d_rs, "d_rs", "uint8", S * cap * ctypes.sizeof(DemodFrameRs), dev)
        _check_dev(d_erec, "d_erec", "uint8", S * cap * ctypes.sizeof(DemodFrameErase), dev)
        rc = self._lib.demod_frames_rs_erasures_async(
            self._h, _ptr(d_rows), _ptr(d_erase), _ptr(d_results), S, cap, N, int(len_bytes), int(crc), int(fec),
            _ptr(d_rs), _ptr(d_erec), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_frames_rs_erasures_async")

    def rx_advance_async(self, d_state, d_ring_sym_in, d_ring_mag_in, d_new_sym, d_new_mag,
                         n_new_windows: int, d_new_first, d_new_count, n_streams: int, ring_windows: int,
                         d_ring_sym_out, d_ring_mag_out, d_first, d_count, stream: int = 0) -> None:
        """demod_rx_advance_async (include/demod.h "receiver", step 1): every
        stream's kept windows and its new ones from ring "in" to ring "out".
        d_state (uint8, n_streams * sizeof(DemodRxStreamState) bytes), the rings
        (uint8 n_streams * ring_windows; float32 that times k), the new batch
        (uint8 n_new_windows, float32 that times k), d_new_first and d_first
        (int64 tensors holding the uint64 tables) and d_new_count and d_count
        (int32 holding uint32) are device tensors, checked like the batch
        calls' (dtype, contiguity, device, size)."""
        S, C, W = int(n_streams), int(ring_windows), int(n_new_windows)
        if S < 1 or S > DEMOD_MAX_SEGMENTS or C < 1 or S * C >= 2 ** 31 or W < 0 or W >= 2 ** 31:
            raise DemodError(DEMOD_BAD_ARG, "n_streams not in 1 .. DEMOD_MAX_SEGMENTS, ring_windows < 1, "
                                            "n_streams * ring_windows >= 2^31 or n_new_windows not in "
                                            "0 .. 2^31 - 1")
        dev = int(self.cfg.device)
        _check_dev(d_state, "d_state", "uint8", S * ctypes.sizeof(DemodRxStreamState), dev)
        _check_dev(d_ring_sym_in, "d_ring_sym_in", "uint8", S * C, dev)
        _check_dev(d_ring_mag_in, "d_ring_mag_in", "float32", S * C * self.k, dev)
        _check_dev(d_new_sym, "d_new_sym", "uint8", max(W, 1), dev)
        _check_dev(d_new_mag, "d_new_mag", "float32", max(W, 1) * self.k, dev)
        _check_dev(d_new_first, "d_new_first", "int64", S, dev)
        _check_dev(d_new_count, "d_new_count", "int32", S, dev)
        _check_dev(d_ring_sym_out, "d_ring_sym_out", "uint8", S * C, dev)
        _check_dev(d_ring_mag_out, "d_ring_mag_out", "float32", S * C * self.k, dev)
        _check_dev(d_first, "d_first", "int64", S, dev)
        _check_dev(d_count, "d_count", "int32", S, dev)
        rc = self._lib.demod_rx_advance_async(
            self._h, _ptr(d_state), _ptr(d_ring_sym_in), _ptr(d_ring_mag_in), _ptr(d_new_sym), _ptr(d_new_mag),
            W, _ptr(d_new_first), _ptr(d_new_count), S, C, _ptr(d_ring_sym_out), _ptr(d_ring_mag_out),
            _ptr(d_first), _ptr(d_count), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_rx_advance_async")

    def rx_collect_async(self, d_state, d_hits, d_results, d_check, d_kept, d_body, d_check_summary,
                         n_streams: int, max_frames: int, sync_len: int, frame_symbols: int, len_bytes: int,
                         crc: int, fec: int, d_frames, d_bodies, d_summary, d_work, stream: int = 0) -> None:
        """demod_rx_collect_async (include/demod.h "receiver", steps 3 and 4)
        over the outputs of frames_segments_async and frames_check_async (fec
        0) or frames_check_coded_async. d_frames (uint8, n_streams * max_frames
        * sizeof(DemodRxFrame) bytes), d_bodies (uint8, n_streams * max_frames
        * max_len bytes), d_summary (uint8, sizeof(DemodRxSummary) bytes) and
        d_state are written; d_work (uint8, at least rx_collect_workspace_size
        bytes) may hold anything. Device tensors, checked like the batch
        calls'."""
        S, cap, N = _rows_shape(n_streams, max_frames, frame_symbols, "n_streams")
        L = int(sync_len)
        if fec != 0 and fec not in RS_MODES:
            raise DemodError(DEMOD_BAD_ARG, "fec: not 0 or one of the 20 modes")
        _, max_len = self._frame_shape(N, len_bytes, crc, fec)
        dev = int(self.cfg.device)
        rows = S * cap
        _check_dev(d_state, "d_state", "uint8", S * ctypes.sizeof(DemodRxStreamState), dev)
        self._check_scan_outputs(S, cap, max_len, d_hits, d_results, d_check, d_kept, d_body, d_check_summary,
                                 collect=True)
        _check_dev(d_frames, "d_frames", "uint8", rows * ctypes.sizeof(DemodRxFrame), dev)
        _check_dev(d_bodies, "d_bodies", "uint8", rows * max_len, dev)
        _check_dev(d_summary, "d_summary", "uint8", ctypes.sizeof(DemodRxSummary), dev)
        _check_dev(d_work, "d_work", "uint8", rx_collect_workspace_size(self.cfg, S), dev)
        rc = self._lib.demod_rx_collect_async(
            self._h, _ptr(d_state), _ptr(d_hits), _ptr(d_results), _ptr(d_check), _ptr(d_kept),
            _ptr(d_body) if d_body is not None else None, _ptr(d_check_summary), S, cap, L, N, int(len_bytes),
            int(crc), int(fec), _ptr(d_frames), _ptr(d_bodies) if d_bodies is not None else None,
            _ptr(d_summary), _ptr(d_work), int(d_work.numel()), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_rx_collect_async")

    def _tx_shape(self, txcfg: DemodTxCfg, n_streams: int) -> dict:
        if n_streams < 1:
            raise DemodError(DEMOD_BAD_ARG, "n_streams < 1")
        return tx_sizes(self.cfg, txcfg, int(n_streams))

    def tx_encode_async(self, txcfg: DemodTxCfg, d_state, d_ring, d_records, d_count, d_bytes, n_bytes: int,
                        n_streams: int, d_place, stream: int = 0) -> None:
        """demod_tx_encode_async (include/demod.h "transmitter", send): two
        launches. d_state (uint8, n_streams * 40 bytes), d_ring (uint8 n_streams
        * ring_symbols), d_records (uint8, n_streams * max_frames * 8 bytes),
        d_count (int32 holding uint32 [n_streams]), d_bytes (uint8 n_bytes, or
        None when n_bytes == 0) and d_place (uint8, n_streams * max_frames * 16
        bytes) are device tensors, checked like the batch calls'."""
        z = self._tx_shape(txcfg, n_streams)
        S, nb = int(n_streams), int(n_bytes)
        if nb < 0 or nb >= 2 ** 32:
            raise DemodError(DEMOD_BAD_ARG, "n_bytes not in 0 .. 2^32 - 1")
        dev = int(self.cfg.device)
        _check_dev(d_state, "d_state", "uint8", z["state_bytes"], dev)
        _check_dev(d_ring, "d_ring", "uint8", z["ring_bytes"], dev)
        _check_dev(d_records, "d_records", "uint8", z["records_bytes"], dev)
        _check_dev(d_count, "d_count", "int32", S, dev)
        _check_dev(d_bytes, "d_bytes", "uint8", max(nb, 1), dev, nullable=nb == 0)
        _check_dev(d_place, "d_place", "uint8", z["places_bytes"], dev)
        rc = self._lib.demod_tx_encode_async(self._h, ctypes.byref(txcfg), _ptr(d_state), _ptr(d_ring),
                                             _ptr(d_records), _ptr(d_count), _ptr(d_bytes), nb, S,
                                             _ptr(d_place), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_tx_encode_async")

    def tx_modulate_async(self, txcfg: DemodTxCfg, d_state, d_ring, d_count, n_streams: int, d_pcm, d_work,
                          stream: int = 0) -> None:
        """demod_tx_modulate_async (include/demod.h "transmitter", modulate):
        three launches. d_pcm is int16 [n_streams * max_samples], d_work uint8 of
        tx_modulate_workspace_size bytes; the rest as tx_encode_async."""
        z = self._tx_shape(txcfg, n_streams)
        S = int(n_streams)
        dev = int(self.cfg.device)
        _check_dev(d_state, "d_state", "uint8", z["state_bytes"], dev)
        _check_dev(d_ring, "d_ring", "uint8", z["ring_bytes"], dev)
        _check_dev(d_count, "d_count", "int32", S, dev)
        _check_dev(d_pcm, "d_pcm", "int16", z["pcm_bytes"] // 2, dev)
        _check_dev(d_work, "d_work", "uint8", z["modulate_work_bytes"], dev)
        rc = self._lib.demod_tx_modulate_async(self._h, ctypes.byref(txcfg), _ptr(d_state), _ptr(d_ring),
                                               _ptr(d_count), S, _ptr(d_pcm), _ptr(d_work),
                                               int(d_work.numel()), stream or None)
        if rc < 0:
            raise DemodError(rc, "demod_tx_modulate_async")

    def frames_checked(self, pcm, sync, max_errors: int = 0, frame_symbols: int = 0, len_bytes: int = 2,
                       crc: int = DEMOD_CRC16_CCITT_FALSE, max_frames: Optional[int] = None,
                       n_windows: Optional[int] = None, body: bool = True):
        """demod_frames_checked: the detector over the sliding windows of pcm (a
        host int16 array or a device tensor), the frame scan and the check of
        its rows. Returns (hits: a FRAME_HIT_DTYPE array [n_kept], lengths
        uint32 [n_kept], bodies: a list of n_kept bytes objects or None, the
        scan's result dict, the check's summary dict): the kept frames alone."""
        return self._frames_checked(pcm, sync, max_errors, frame_symbols, len_bytes, crc, 0, max_frames,
                                    n_windows, body)

    def frames_coded(self, pcm, sync, max_errors: int = 0, frame_symbols: int = 0, len_bytes: int = 2,
                     crc: int = DEMOD_CRC16_CCITT_FALSE, fec: int = DEMOD_FEC_CONV_K7,
                     max_frames: Optional[int] = None, n_windows: Optional[int] = None, body: bool = True):
        """demod_frames_coded: frames_checked for coded frames (include/demod.h
        "coded frames"): detector, frame scan, soft-decision decode of its rows
        and the coded check; with a parity flag the Reed-Solomon stage before
        the check, and with fec & 0xFF == 0 over the scan's packed rows.
        Returns what frames_checked returns."""
        erase_mode_parts(fec)   # alone here: with or without DEMOD_FEC_ERASE(level)
        return self._frames_checked(pcm, sync, max_errors, frame_symbols, len_bytes, crc, int(fec), max_frames,
                                    n_windows, body)

    def _frames_checked(self, pcm, sync, max_errors, frame_symbols, len_bytes, crc, fec, max_frames,
                        n_windows, body):
        """frames_checked (fec 0) and frames_coded."""
        buf, n_windows = self._stage(pcm, n_windows)
        sync = _sync_bytes(sync)
        N = int(frame_symbols)
        if N < 0 or (max_frames is not None and max_frames < 1):
            raise DemodError(DEMOD_BAD_ARG, "frame_symbols < 0 or max_frames < 1")
        _, max_len = self._frame_shape(N, len_bytes, crc, fec & ~(0x7F << 16))
        if max_frames is None:
            max_frames = n_windows // max(self.n // self.hop, 1) + 1
        cap = int(max_frames)
        hits = np.zeros(cap, dtype=FRAME_HIT_DTYPE)
        lengths = np.zeros(cap, dtype=np.uint32)
        bod = np.zeros((cap, max(max_len, 1)), dtype=np.uint8) if body else None
        res, summ = DemodFramesResult(), DemodFramesCheckResult()
        head = (self._h, _ptr(buf), n_windows, _ptr(sync) if sync.size else None, sync.size, int(max_errors), N,
                int(len_bytes), int(crc))
        tail = (_ptr(hits), _ptr(lengths), _ptr(bod) if bod is not None and max_len else None, cap,
                ctypes.byref(res), ctypes.byref(summ))
        if fec:
            rc = self._lib.demod_frames_coded(*head, fec, *tail)
        else:
            rc = self._lib.demod_frames_checked(*head, *tail)
        if rc < 0:
            raise DemodError(rc, "demod_frames_coded" if fec else "demod_frames_checked")
        bodies = [bytes(bod[r, :int(lengths[r])]) for r in range(rc)] if bod is not None else None
        summary = _struct_dict(summ)
        return hits[:rc], lengths[:rc], bodies, frames_result_dict(res), summary


def _packet_tables(packets, S: int, ch: int):
    """One packet per stream -> (the arrays kept alive, ptrs uintp [S], frames
    uintp [S]), as demod_streams_push and demod_rx_push take them."""
    if isinstance(packets, np.ndarray) and packets.ndim == 2:
        if packets.shape[0] != S:
            raise DemodError(DEMOD_BAD_ARG, "one packet row per stream")
        rows_ok = (packets.dtype == np.int16 and packets.strides[0] >= 0
                   and (packets.shape[1] <= 1 or packets.strides[1] == 2))
        # rows need only be contiguous each (a column slice of a longer
        # recording is not copied)
        keep = packets if rows_ok else np.ascontiguousarray(packets, dtype=np.int16)
        if keep.shape[1] % ch:
            raise DemodError(DEMOD_BAD_ARG, "pcm length not a multiple of channels")
        frames = np.full(S, keep.shape[1] // ch, dtype=np.uintp)
        ptrs = np.zeros(S, dtype=np.uintp)
        if keep.shape[1]:
            ptrs += np.uintp(keep.ctypes.data)
            ptrs += np.arange(S, dtype=np.uintp) * np.uintp(keep.strides[0])
    else:
        if len(packets) != S:
            raise DemodError(DEMOD_BAD_ARG, "one packet (or None) per stream")
        keep = [np.ascontiguousarray(p, dtype=np.int16) if p is not None else None for p in packets]
        frames = np.array([0 if a is None else a.size // ch for a in keep], dtype=np.uintp)
        for a in keep:
            if a is not None and a.size % ch:
                raise DemodError(DEMOD_BAD_ARG, "pcm length not a multiple of channels")
        ptrs = np.array([0 if a is None or a.size == 0 else a.ctypes.data for a in keep],
                        dtype=np.uintp)
    return keep, ptrs, frames


class Streams(_Handle):
    """demod_streams_t: n_streams independent streams behind one detector,
    one batch per push (include/demod.h, "many streams, one launch")."""
    _destroy = "demod_streams_destroy"

    def __init__(self, n_streams: int, cfg: Optional[DemodCfg] = None, **kw):
        self._lib = load_library()
        self.cfg = cfg if cfg is not None else make_cfg(**kw)
        self.n_streams = int(n_streams)
        err = ctypes.c_int(0)
        h = self._lib.demod_streams_create(ctypes.byref(self.cfg), self.n_streams, ctypes.byref(err))
        if not h:
            raise DemodError(err.value, "demod_streams_create")
        self._h = h

    @property
    def k(self) -> int:
        return int(self.cfg.k)

    def reset(self, stream: int) -> None:
        rc = self._lib.demod_streams_reset(self._h, int(stream))
        if rc < 0:
            raise DemodError(rc, "demod_streams_reset")

    def pending(self, stream: int) -> int:
        rc = self._lib.demod_streams_pending(self._h, int(stream))
        if rc < 0:
            raise DemodError(rc, "demod_streams_pending")
        return rc

    def push(self, packets, mags: bool = False, cap: Optional[int] = None):
        """packets: one int16 array (interleaved if stereo) or None per stream,
        or one 2-D array whose rows are the streams' packets (equal lengths;
        its row addresses are computed, not read array by array).
        Returns the per-stream symbol arrays (and magnitude arrays)."""
        S = self.n_streams
        keep, ptrs, frames = _packet_tables(packets, S, int(self.cfg.channels))
        if cap is None:
            cap = int(self._lib.demod_streams_max_symbols(self._h, frames.ctypes.data))
        sym = np.empty(max(cap, 1), dtype=np.uint8)
        mag = np.empty((max(cap, 1), self.k), dtype=np.float32) if mags else None
        counts = np.zeros(S, dtype=np.uint32)
        rc = self._lib.demod_streams_push(self._h, ptrs.ctypes.data, frames.ctypes.data,
                                          _ptr(sym), _ptr(mag), cap, counts.ctypes.data)
        del keep
        if rc < 0:
            raise DemodError(rc, "demod_streams_push")
        e = [0] + np.cumsum(counts, dtype=np.int64).tolist()
        out_s = [sym[e[i]:e[i + 1]] for i in range(S)]
        if not mags:
            return out_s
        return out_s, [mag[e[i]:e[i + 1]] for i in range(S)]


class Receiver(_Handle):
    """demod_rx_t: n_streams live streams in, their checked (or decoded and
    checked) frames out, the carry between packets kept on the device
    (include/demod.h "receiver")."""
    _destroy = "demod_rx_destroy"

    def __init__(self, n_streams: int, rxcfg: DemodRxCfg, cfg: Optional[DemodCfg] = None, **kw):
        self._lib = load_library()
        self.cfg = cfg if cfg is not None else make_cfg(**kw)
        self.rxcfg = rxcfg
        self.n_streams = int(n_streams)
        self.sizes = rx_sizes(self.cfg, rxcfg, self.n_streams)
        err = ctypes.c_int(0)
        h = self._lib.demod_rx_create(ctypes.byref(self.cfg), ctypes.byref(rxcfg), self.n_streams,
                                      ctypes.byref(err))
        if not h:
            raise DemodError(err.value, "demod_rx_create")
        self._h = h

    def reset(self, stream: int) -> None:
        rc = self._lib.demod_rx_reset(self._h, int(stream))
        if rc < 0:
            raise DemodError(rc, "demod_rx_reset")

    def state(self, stream: int) -> dict:
        """The stream's demod_rx_stream_state_t after the last push."""
        if stream < 0:
            raise DemodError(DEMOD_BAD_ARG, "demod_rx_state")
        st = DemodRxStreamState()
        rc = self._lib.demod_rx_state(self._h, int(stream), ctypes.byref(st))
        if rc < 0:
            raise DemodError(rc, "demod_rx_state")
        return _struct_dict(st)

    def push(self, packets):
        """packets as Streams.push takes them. Returns (frames: an
        RX_FRAME_DTYPE array [n_frames], copied out of the handle's memory,
        bodies: a list of n_frames bytes objects, the summary dict)."""
        keep, ptrs, nfr = _packet_tables(packets, self.n_streams, int(self.cfg.channels))
        frames, bodies, summ = _P(), _P(), DemodRxSummary()
        rc = self._lib.demod_rx_push(self._h, ptrs.ctypes.data, nfr.ctypes.data, ctypes.byref(frames),
                                     ctypes.byref(bodies), ctypes.byref(summ))
        del keep
        if rc < 0:
            raise DemodError(rc, "demod_rx_push")
        summary = _struct_dict(summ)
        rec = np.zeros(rc, RX_FRAME_DTYPE)
        if rc:
            ctypes.memmove(rec.ctypes.data, frames.value, rc * RX_FRAME_DTYPE.itemsize)
        raw = ctypes.string_at(bodies.value, summary["n_bytes"]) if summary["n_bytes"] else b""
        out = [raw[int(r["body"]):int(r["body"]) + int(r["length"])] for r in rec]
        return rec, out, summary


class Transmitter(_Handle):
    """demod_tx_t: frames in, as Receiver.push hands them out, and the
    phase-continuous signal of n_streams streams out; queues and phases are
    kept on the device (include/demod.h "transmitter")."""
    _destroy = "demod_tx_destroy"

    def __init__(self, n_streams: int, txcfg: DemodTxCfg, cfg: Optional[DemodCfg] = None, **kw):
        self._lib = load_library()
        self.cfg = cfg if cfg is not None else make_cfg(**kw)
        self.txcfg = txcfg
        self.n_streams = int(n_streams)
        self.sizes = tx_sizes(self.cfg, txcfg, self.n_streams)
        err = ctypes.c_int(0)
        h = self._lib.demod_tx_create(ctypes.byref(self.cfg), ctypes.byref(txcfg), self.n_streams,
                                      ctypes.byref(err))
        if not h:
            raise DemodError(err.value, "demod_tx_create")
        self._h = h

    def reset(self, stream: int) -> None:
        rc = self._lib.demod_tx_reset(self._h, int(stream)) if stream >= 0 else DEMOD_BAD_ARG
        if rc < 0:
            raise DemodError(rc, "demod_tx_reset")

    def state(self, stream: int) -> dict:
        """The stream's demod_tx_stream_state_t after the last send or pull."""
        if stream < 0:
            raise DemodError(DEMOD_BAD_ARG, "demod_tx_state")
        st = DemodTxStreamState()
        rc = self._lib.demod_tx_state(self._h, int(stream), ctypes.byref(st))
        if rc < 0:
            raise DemodError(rc, "demod_tx_state")
        return _struct_dict(st)

    def device_buffers(self) -> Tuple[int, int]:
        """The device addresses of the last pull's samples [S][max_samples] and of the ring."""
        pcm, ring = _P(), _P()
        rc = self._lib.demod_tx_device_buffers(self._h, ctypes.byref(pcm), ctypes.byref(ring))
        if rc < 0:
            raise DemodError(rc, "demod_tx_device_buffers")
        return int(pcm.value), int(ring.value)

    def device_pcm(self):
        """The last pull's samples on the device, a torch int16 tensor
        [n_streams * max_samples] over the handle's own memory (no copy): what
        demod_batch_async takes. Valid until the handle is closed."""
        import torch

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (self.n_streams * int(self.txcfg.max_samples),), "typestr": "<i2",
                                      "data": (self.device_buffers()[0], False), "version": 2}
        return torch.as_tensor(v, device=f"cuda:{int(self.cfg.device)}")

    def send(self, frames, bodies: bytes = b""):
        """frames: an RX_FRAME_DTYPE array as Receiver.push returns it (stream,
        length and body are read) with bodies the dense bytes, or a list of
        (stream, bytes) pairs. Returns (accepted, places: a TX_PLACE_DTYPE
        array in input order)."""
        if not isinstance(frames, np.ndarray):
            pairs = [(int(s), bytes(b)) for s, b in frames]
            rec = np.zeros(len(pairs), RX_FRAME_DTYPE)
            off = 0
            for i, (s, b) in enumerate(pairs):
                rec[i]["stream"], rec[i]["length"], rec[i]["body"] = s, len(b), off
                off += len(b)
            frames, bodies = rec, b"".join(b for _, b in pairs)
        rec = np.ascontiguousarray(frames, dtype=RX_FRAME_DTYPE)
        bodies = bytes(bodies)
        buf = ctypes.create_string_buffer(bodies, max(len(bodies), 1))
        place = np.zeros(rec.size, TX_PLACE_DTYPE)
        rc = self._lib.demod_tx_send(self._h, rec.ctypes.data if rec.size else None, rec.size,
                                     ctypes.addressof(buf), len(bodies), place.ctypes.data if rec.size else None)
        if rc < 0:
            raise DemodError(rc, "demod_tx_send")
        return rc, place

    def pull(self, n_frames) -> list:
        """n_frames: one count for every stream, or a sequence of n_streams
        counts. Returns the streams' int16 sample arrays."""
        S = self.n_streams
        counts = [int(n_frames)] * S if np.isscalar(n_frames) else [int(v) for v in n_frames]
        if len(counts) != S or min(counts) < 0:
            raise DemodError(DEMOD_BAD_ARG, "one non-negative count per stream")
        out = [np.empty(c, np.int16) for c in counts]
        nfr = np.asarray(counts, dtype=np.uintp)
        ptrs = np.asarray([a.ctypes.data if a.size else 0 for a in out], dtype=np.uintp)
        rc = self._lib.demod_tx_pull(self._h, nfr.ctypes.data, ptrs.ctypes.data)
        if rc < 0:
            raise DemodError(rc, "demod_tx_pull")
        return out


# demod_decode_fn: opus_decode's signature (opus.h:462)
DECODE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                             ctypes.c_void_p, ctypes.c_int, ctypes.c_int)


def push_packets(streams: "Streams", decode, decoders: Sequence[int], packets: Sequence[Optional[bytes]],
                 frame_size: int, mags: bool = False, cap: Optional[int] = None):
    """demod_streams_push_packets: one encoded packet per stream (bytes, or
    None / b"" for none), decoded by `decode` (a DECODE_FN, or the address of
    a native demod_decode_fn such as opus_decode) with decoders[i] (a state
    pointer) into PCM, then pushed. Returns the per-stream symbol arrays (and
    magnitude arrays)."""
    lib = streams._lib
    S = streams.n_streams
    if len(packets) != S or len(decoders) != S:
        raise DemodError(DEMOD_BAD_ARG, "one packet and one decoder per stream")
    bufs = [ctypes.create_string_buffer(bytes(p), max(len(p), 1)) if p else None for p in packets]
    pk = (ctypes.c_void_p * S)(*[ctypes.addressof(b) if b is not None else None for b in bufs])
    lens = (ctypes.c_int32 * S)(*[len(p) if p else 0 for p in packets])
    decs = (ctypes.c_void_p * S)(*decoders)
    if cap is None:
        frames = np.full(S, frame_size, dtype=np.uintp)
        cap = int(lib.demod_streams_max_symbols(streams._h, frames.ctypes.data))
    sym = np.empty(max(cap, 1), dtype=np.uint8)
    mag = np.empty((max(cap, 1), streams.k), dtype=np.float32) if mags else None
    counts = np.zeros(S, dtype=np.uint32)
    fn = ctypes.cast(decode, ctypes.c_void_p) if not isinstance(decode, int) else ctypes.c_void_p(decode)
    rc = lib.demod_streams_push_packets(streams._h, fn, decs, pk, lens, int(frame_size), _ptr(sym),
                                        _ptr(mag), cap, counts.ctypes.data)
    del bufs
    if rc < 0:
        raise DemodError(rc, "demod_streams_push_packets")
    e = [0] + np.cumsum(counts, dtype=np.int64).tolist()
    out_s = [sym[e[i]:e[i + 1]] for i in range(S)]
    if not mags:
        return out_s
    return out_s, [mag[e[i]:e[i + 1]] for i in range(S)]


def synth_fsk(cfg: DemodCfg, seed: int, n_windows: int, amplitude: int, sigma: int,
              d_pcm, d_sym=None, stream: int = 0, w0: int = 0) -> None:
    """Device generator of the seeded FSK test signal into device buffers."""
    _check_dev(d_pcm, "d_pcm", "int16", int(n_windows) * int(cfg.n), int(cfg.device))
    _check_dev(d_sym, "d_sym", "uint8", int(n_windows), int(cfg.device), nullable=True)
    rc = load_library().demod_synth_fsk(ctypes.byref(cfg), ctypes.c_uint64(seed),
                                         ctypes.c_uint64(w0), n_windows,
                                         amplitude, sigma, _ptr(d_pcm), _ptr(d_sym),
                                         stream or None)
    if rc < 0:
        raise DemodError(rc, "demod_synth_fsk")


def read_ceiling_async(d_buf, n_bytes: int, stream: int = 0) -> None:
    """Read-only reference stream over a device buffer (demod_read_ceiling_async)."""
    if not hasattr(d_buf, "numel") or d_buf.numel() * d_buf.element_size() < n_bytes:
        raise DemodError(DEMOD_BAD_ARG, "read_ceiling_async: buffer smaller than n_bytes")
    rc = load_library().demod_read_ceiling_async(_ptr(d_buf), n_bytes, stream or None)
    if rc < 0:
        raise DemodError(rc, "demod_read_ceiling_async")


# ---- ip.proto framing (host) ---------------------------------------------

def frame_size(payload_len: int) -> int:
    return int(load_library().demod_frame_size(payload_len))


def frame_encode(payload: bytes) -> bytes:
    lib = load_library()
    src = (ctypes.c_uint8 * max(len(payload), 1)).from_buffer_copy(payload or b"\0")
    cap = lib.demod_frame_size(len(payload))
    out = (ctypes.c_uint8 * cap)()
    rc = lib.demod_frame_encode(src, len(payload), out, cap)
    if rc < 0:
        raise DemodError(rc, "demod_frame_encode")
    return bytes(out[:rc])


def crc(kind: int, data: bytes) -> int:
    """demod_crc: DEMOD_CRC16_CCITT_FALSE or DEMOD_CRC32_MPEG2 of data."""
    if kind not in CRC_BYTES:
        raise DemodError(DEMOD_BAD_ARG, "crc: unknown kind")
    data = bytes(data)
    src = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    return int(load_library().demod_crc(kind, src, len(data)))


def checked_frame_size(length: int, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE) -> int:
    """demod_checked_frame_size: len_bytes + length + the CRC's bytes."""
    rc = int(load_library().demod_checked_frame_size(int(length), int(len_bytes), int(crc)))
    if rc < 0:
        raise DemodError(rc, "demod_checked_frame_size")
    return rc


def checked_frame_encode(data: bytes, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                         cap: Optional[int] = None) -> bytes:
    """demod_checked_frame_encode: len || data || CRC (include/demod.h "checked
    frames"); unpack_symbols turns the bytes into symbols. cap: the output
    room handed to the library (default: what the frame needs)."""
    lib = load_library()
    data = bytes(data)
    if cap is None:
        cap = len(data) + 8
    src = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (ctypes.c_uint8 * max(int(cap), 1))()
    rc = lib.demod_checked_frame_encode(src, len(data), int(len_bytes), int(crc), out, int(cap))
    if rc < 0:
        raise DemodError(rc, "demod_checked_frame_encode")
    return bytes(out[:rc])


def coded_frame_steps(length: int, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE) -> int:
    """demod_coded_frame_steps: T(len), the trellis steps of a coded frame."""
    rc = int(load_library().demod_coded_frame_steps(int(length), int(len_bytes), int(crc)))
    if rc < 0:
        raise DemodError(rc, "demod_coded_frame_steps")
    return rc


def coded_frame_symbols(length: int, len_bytes: int, crc: int, bits: int) -> int:
    """demod_coded_frame_symbols: Sc = ceil(2 T(len) / bits)."""
    rc = int(load_library().demod_coded_frame_symbols(int(length), int(len_bytes), int(crc), int(bits)))
    if rc < 0:
        raise DemodError(rc, "demod_coded_frame_symbols")
    return rc


def coded_frame_encode(data: bytes, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                       cap: Optional[int] = None) -> bytes:
    """demod_coded_frame_encode: the coded bits of len || data || CRC (include/
    demod.h "coded frames"); unpack_symbols turns the bytes into symbols. cap:
    the output room handed to the library (default: what the frame needs)."""
    lib = load_library()
    data = bytes(data)
    if cap is None:
        cap = 2 * len(data) + 32
    src = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (ctypes.c_uint8 * max(int(cap), 1))()
    rc = lib.demod_coded_frame_encode(src, len(data), int(len_bytes), int(crc), out, int(cap))
    if rc < 0:
        raise DemodError(rc, "demod_coded_frame_encode")
    return bytes(out[:rc])


def coded_row_bytes(frame_symbols: int, bits: int, len_bytes: int = 2) -> int:
    """demod_coded_row_bytes: Bd, the decoded bytes of rows of frame_symbols symbols."""
    if frame_symbols < 0:
        raise DemodError(DEMOD_BAD_ARG, "demod_coded_row_bytes")
    rc = int(load_library().demod_coded_row_bytes(int(frame_symbols), int(bits), int(len_bytes)))
    if rc < 0:
        raise DemodError(rc, "demod_coded_row_bytes")
    return rc


def soft_bits(powers) -> np.ndarray:
    """demod_soft_bits: the int8 soft values [bits] of one window's K powers."""
    p = np.ascontiguousarray(powers, dtype=np.float32).reshape(-1)
    out = np.zeros(8, dtype=np.int8)
    rc = load_library().demod_soft_bits(_ptr(p) if p.size else None, p.size, _ptr(out))
    if rc < 0:
        raise DemodError(rc, "demod_soft_bits")
    return out[:rc].copy()


def pack_mask(flags, row_bytes: int) -> np.ndarray:
    """A bool a row byte -> the row's Wm uint64 mask words (byte b is bit b & 63
    of word b >> 6; bits at b >= row_bytes 0)."""
    f = np.zeros(mask_words(row_bytes) * 64, dtype=np.uint8)
    src = np.asarray(flags, dtype=bool).reshape(-1)[:int(row_bytes)]
    f[:src.size] = src
    return np.packbits(f, bitorder="little").view("<u8").astype(np.uint64)


def soft_erasures(soft, level: int, row_bytes: int) -> np.ndarray:
    """demod_soft_erasures: the Wm uint64 mask words of one plain row from its
    int8 soft values in air order."""
    q = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1)
    if int(row_bytes) < 1 or int(row_bytes) >= 2 ** 31:
        raise DemodError(DEMOD_BAD_ARG, "row_bytes not in 1 .. 2^31 - 1")
    out = np.zeros(mask_words(row_bytes), dtype=np.uint64)
    keep = q if q.size else np.zeros(1, dtype=np.int8)
    rc = load_library().demod_soft_erasures(keep.ctypes.data, q.size, int(level), out.ctypes.data, int(row_bytes))
    if rc < 0:
        raise DemodError(rc, "demod_soft_erasures")
    return out


def coded_frame_decode(soft, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                       cap: Optional[int] = None) -> Tuple[bytes, dict]:
    """demod_coded_frame_decode: the host decoder on int8 soft values. Returns
    (the row bytes written, the decode record as a dict). cap: the row room
    handed to the library (default: Bd)."""
    q = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1)
    if cap is None:
        cap = max((q.size // 2 - 6) // 8, 0)
    row = np.zeros(max(int(cap), 1), dtype=np.uint8)
    dec = DemodFrameDecode()
    rc = load_library().demod_coded_frame_decode(_ptr(q) if q.size else None, q.size, int(len_bytes),
                                                 int(crc), _ptr(row), int(cap), ctypes.byref(dec))
    if rc < 0:
        raise DemodError(rc, "demod_coded_frame_decode")
    return row[:rc].tobytes(), _struct_dict(dec)


def fec_air_index(fec: int, m: int) -> int:
    """demod_fec_air_index: the air position of mother bit m = 2 t + v in the
    mode `fec`, or -1 where it is punctured."""
    if fec not in RS_CONV_MODES or not 0 <= int(m) < 2 ** 31:
        raise DemodError(DEMOD_BAD_ARG, "demod_fec_air_index")
    return int(load_library().demod_fec_air_index(int(fec), int(m)))


def fec_frame_symbols(length: int, len_bytes: int, crc: int, bits: int, fec: int) -> int:
    """demod_fec_frame_symbols: Sc of the mode, ceil(Na(len) / bits)."""
    if fec not in RS_CONV_MODES:
        raise DemodError(DEMOD_BAD_ARG, "demod_fec_frame_symbols")
    rc = int(load_library().demod_fec_frame_symbols(int(length), int(len_bytes), int(crc), int(bits), int(fec)))
    if rc < 0:
        raise DemodError(rc, "demod_fec_frame_symbols")
    return rc


def fec_frame_encode(data: bytes, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                     fec: int = DEMOD_FEC_CONV_K7, cap: Optional[int] = None) -> bytes:
    """demod_fec_frame_encode: the frame's bits in air order, pad bits 0. cap:
    the output room handed to the library (default: what any mode needs)."""
    if fec not in RS_CONV_MODES:
        raise DemodError(DEMOD_BAD_ARG, "demod_fec_frame_encode")
    lib = load_library()
    data = bytes(data)
    if cap is None:
        cap = 2 * len(data) + 64
        if fec & (DEMOD_FEC_RS16 | DEMOD_FEC_RS32):   # twice the n' bytes, and the same slack
            cap = 2 * rs_frame_size(len(data), len_bytes, crc, fec) + 64
    src = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    out = (ctypes.c_uint8 * max(int(cap), 1))()
    rc = lib.demod_fec_frame_encode(src, len(data), int(len_bytes), int(crc), int(fec), out, int(cap))
    if rc < 0:
        raise DemodError(rc, "demod_fec_frame_encode")
    return bytes(out[:rc])


def fec_row_bytes(frame_symbols: int, bits: int, len_bytes: int = 2, fec: int = DEMOD_FEC_CONV_K7) -> int:
    """demod_fec_row_bytes: Bd of rows of frame_symbols symbols in the mode."""
    if frame_symbols < 0 or fec not in RS_CONV_MODES:
        raise DemodError(DEMOD_BAD_ARG, "demod_fec_row_bytes")
    rc = int(load_library().demod_fec_row_bytes(int(frame_symbols), int(bits), int(len_bytes), int(fec)))
    if rc < 0:
        raise DemodError(rc, "demod_fec_row_bytes")
    return rc


def fec_frame_decode(soft, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                     fec: int = DEMOD_FEC_CONV_K7, cap: Optional[int] = None) -> Tuple[bytes, dict]:
    """demod_fec_frame_decode: the host decoder on int8 soft values in air
    order. Returns (the row bytes written, the decode record as a dict). cap:
    the row room handed to the library (default: Bd)."""
    q = np.ascontiguousarray(soft, dtype=np.int8).reshape(-1)
    if cap is None:
        if fec not in RS_CONV_MODES:
            raise DemodError(DEMOD_BAD_ARG, "demod_fec_frame_decode")
        cap = max((fec_row_steps(q.size, fec & 0xFF) - 6) // 8, 0)
    elif fec not in RS_CONV_MODES:
        raise DemodError(DEMOD_BAD_ARG, "demod_fec_frame_decode")
    row = np.zeros(max(int(cap), 1), dtype=np.uint8)
    dec = DemodFrameDecode()
    rc = load_library().demod_fec_frame_decode(_ptr(q) if q.size else None, q.size, int(len_bytes), int(crc),
                                               int(fec), _ptr(row), int(cap), ctypes.byref(dec))
    if rc < 0:
        raise DemodError(rc, "demod_fec_frame_decode")
    return row[:rc].tobytes(), _struct_dict(dec)


def rs_generator(parity_bytes: int) -> bytes:
    """demod_rs_generator: g(x) of parity_bytes roots, highest coefficient first."""
    out = (ctypes.c_uint8 * 33)()
    n = load_library().demod_rs_generator(int(parity_bytes), out)
    if n < 0:
        raise DemodError(n, "demod_rs_generator")
    return bytes(out[:n])


def rs_encode(msg: bytes, parity_bytes: int) -> bytes:
    """demod_rs_encode: the parity of one codeword's message."""
    msg = bytes(msg)
    out = (ctypes.c_uint8 * 32)()
    n = load_library().demod_rs_encode(msg, len(msg), int(parity_bytes), out)
    if n < 0:
        raise DemodError(n, "demod_rs_encode")
    return bytes(out[:n])


def rs_frame_size(length: int, len_bytes: int, crc: int, fec: int) -> int:
    """demod_rs_frame_size: n'(len) of the mode."""
    n = load_library().demod_rs_frame_size(int(length), int(len_bytes), int(crc), int(fec))
    if n < 0:
        raise DemodError(int(n), "demod_rs_frame_size")
    return int(n)


def rs_max_len(row_bytes: int, len_bytes: int, crc: int, fec: int) -> int:
    """demod_rs_max_len: the greatest len whose protected frame fits a row."""
    if row_bytes < 0:
        raise DemodError(DEMOD_BAD_ARG, "row_bytes < 0")
    n = load_library().demod_rs_max_len(int(row_bytes), int(len_bytes), int(crc), int(fec))
    if n < 0:
        raise DemodError(int(n), "demod_rs_max_len")
    return int(n)


def rs_frame_encode(data: bytes, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE,
                    fec: int = DEMOD_FEC_RS16) -> bytes:
    """demod_rs_frame_encode: len || data || CRC || parity, n' bytes."""
    data = bytes(data)
    cap = rs_frame_size(len(data), len_bytes, crc, fec)
    out = (ctypes.c_uint8 * max(cap, 1))()
    n = load_library().demod_rs_frame_encode(data, len(data), int(len_bytes), int(crc), int(fec), out, cap)
    if n < 0:
        raise DemodError(n, "demod_rs_frame_encode")
    return bytes(out[:n])


def rs_frame_decode(row, len_bytes: int = 2, crc: int = DEMOD_CRC16_CCITT_FALSE, fec: int = DEMOD_FEC_RS16,
                    erase=None):
    """demod_rs_frame_decode on a copy of `row` (bytes or uint8 array; its
    length is the row width): (the corrected row, the record as a dict, the
    bytes covered). With erase (the row's Wm uint64 mask words, or a bool
    array a row byte) demod_rs_frame_decode_erasures: (the corrected row, the
    record, the erasure record, the bytes covered)."""
    buf = np.array(np.frombuffer(bytes(row), np.uint8) if isinstance(row, (bytes, bytearray)) else row,
                   dtype=np.uint8).reshape(-1).copy()
    if buf.size == 0:
        raise DemodError(DEMOD_BAD_ARG, "row: empty")
    rec = DemodFrameRs()
    if erase is not None:
        words = np.asarray(erase)
        words = pack_mask(words, buf.size) if words.dtype == np.bool_ else \
            np.ascontiguousarray(words, dtype=np.uint64).reshape(-1)
        if words.size < mask_words(buf.size):
            raise DemodError(DEMOD_BAD_ARG, "erase: fewer than Wm words")
        erec = DemodFrameErase()
        n = load_library().demod_rs_frame_decode_erasures(buf.ctypes.data, buf.size, int(len_bytes), int(crc),
                                                          int(fec), words.ctypes.data, ctypes.byref(rec),
                                                          ctypes.byref(erec))
        if n < 0:
            raise DemodError(n, "demod_rs_frame_decode_erasures")
        return buf, _struct_dict(rec), _struct_dict(erec), n
    n = load_library().demod_rs_frame_decode(buf.ctypes.data, buf.size, int(len_bytes), int(crc), int(fec),
                                             ctypes.byref(rec))
    if n < 0:
        raise DemodError(n, "demod_rs_frame_decode")
    return buf, _struct_dict(rec), n


def frame_decode(buf: bytes) -> Tuple[bytes, int]:
    """Decode one delimited ToReceiver frame -> (payload, bytes consumed)."""
    lib = load_library()
    src = (ctypes.c_uint8 * max(len(buf), 1)).from_buffer_copy(buf or b"\0")
    pl = ctypes.c_void_p()
    pl_len = _SZ()
    used = _SZ()
    rc = lib.demod_frame_decode(src, len(buf), ctypes.byref(pl), ctypes.byref(pl_len),
                                ctypes.byref(used))
    if rc < 0:
        raise DemodError(rc, "demod_frame_decode")
    off = (pl.value or ctypes.addressof(src)) - ctypes.addressof(src)
    return bytes(buf[off:off + pl_len.value]), int(used.value)


# ---- ip.proto session messages (host; include/demod.h, demod_session.c) ----

def _discovery_struct(d: dict) -> DemodDiscovery:
    s = DemodDiscovery()
    s.protocol_version = int(d.get("protocol_version", 1))
    s.mac_address = int(d.get("mac_address", 0))
    s.device_name = bytes(d.get("device_name", b""))
    s.currently_streaming = int(bool(d.get("currently_streaming", False)))
    s.opus_version = bytes(d.get("opus_version", b""))
    return s


def _discovery_dict(s: DemodDiscovery) -> dict:
    return {"protocol_version": int(s.protocol_version), "mac_address": int(s.mac_address),
            "device_name": bytes(s.device_name), "currently_streaming": bool(s.currently_streaming),
            "opus_version": bytes(s.opus_version)}


def _session_call(fn, name, *args, cap=1024) -> bytes:
    out = (ctypes.c_uint8 * cap)()
    rc = fn(*args, out, cap)
    if rc < 0:
        raise DemodError(rc, name)
    return bytes(out[:rc])


def broadcast_request_encode() -> bytes:
    """BroadcastMessage{magic, discovery_request = true} (discovery.kt:44-48)."""
    return _session_call(load_library().demod_broadcast_request_encode,
                         "demod_broadcast_request_encode")


def broadcast_response_encode(d: dict) -> bytes:
    """BroadcastMessage{magic, discovery_response = d} (network.cpp:356-378)."""
    s = _discovery_struct(d)
    return _session_call(load_library().demod_broadcast_response_encode,
                         "demod_broadcast_response_encode", ctypes.byref(s))


def broadcast_decode(buf: bytes):
    """-> (which, magic, discovery dict or None); DemodError where nanopb fails."""
    lib = load_library()
    src = (ctypes.c_uint8 * max(len(buf), 1)).from_buffer_copy(buf or b"\0")
    magic = ctypes.c_uint32()
    d = DemodDiscovery()
    rc = lib.demod_broadcast_decode(src, len(buf), ctypes.byref(magic), ctypes.byref(d))
    if rc < 0:
        raise DemodError(rc, "demod_broadcast_decode")
    return rc, int(magic.value), (_discovery_dict(d) if rc == DEMOD_MSG_DISCOVERY_RESPONSE
                                  else None)


def hello_encode(info: dict) -> bytes:
    """Delimited ToTransmitter{receiver_information} (network.cpp:388-403)."""
    s = DemodReceiverInfo()
    s.discovery_data = _discovery_struct(info.get("discovery_data", {}))
    s.max_encoded_frame_size = int(info.get("max_encoded_frame_size", DEMOD_MAX_FRAME_PAYLOAD))
    s.max_decoded_frame_size = int(info.get("max_decoded_frame_size", DEMOD_MAX_DECODED_FRAME))
    return _session_call(load_library().demod_hello_encode, "demod_hello_encode",
                         ctypes.byref(s))


def receiver_error_encode(audio_underflow: bool, audio_decode_error: bool) -> bytes:
    """Delimited ToTransmitter{error}."""
    s = DemodReceiverError(int(bool(audio_underflow)), int(bool(audio_decode_error)))
    return _session_call(load_library().demod_receiver_error_encode,
                         "demod_receiver_error_encode", ctypes.byref(s))


def to_transmitter_decode(buf: bytes):
    """Delimited ToTransmitter -> (which, fields dict or None, bytes consumed)."""
    lib = load_library()
    src = (ctypes.c_uint8 * max(len(buf), 1)).from_buffer_copy(buf or b"\0")
    info = DemodReceiverInfo()
    err = DemodReceiverError()
    used = _SZ()
    rc = lib.demod_to_transmitter_decode(src, len(buf), ctypes.byref(info), ctypes.byref(err),
                                         ctypes.byref(used))
    if rc < 0:
        raise DemodError(rc, "demod_to_transmitter_decode")
    if rc == DEMOD_MSG_RECEIVER_INFORMATION:
        fields = {"discovery_data": _discovery_dict(info.discovery_data),
                  "max_encoded_frame_size": int(info.max_encoded_frame_size),
                  "max_decoded_frame_size": int(info.max_decoded_frame_size)}
    elif rc == DEMOD_MSG_RECEIVER_ERROR:
        fields = {"audio_underflow": bool(err.audio_underflow),
                  "audio_decode_error": bool(err.audio_decode_error)}
    else:
        fields = None
    return rc, fields, int(used.value)


def bits_per_symbol(k: int) -> int:
    return int(load_library().demod_bits_per_symbol(k))


def pack_symbols(symbols: np.ndarray, bits: int) -> bytes:
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    cap = (sym.size * bits + 7) // 8
    out = np.empty(max(cap, 1), dtype=np.uint8)
    rc = load_library().demod_pack_symbols(_ptr(sym), sym.size, bits, _ptr(out), cap)
    if rc < 0:
        raise DemodError(rc, "demod_pack_symbols")
    return out[:rc].tobytes()


def unpack_symbols(data: bytes, n: int, bits: int) -> np.ndarray:
    src = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
    if len(data) * 8 < n * bits:
        raise DemodError(DEMOD_BAD_ARG, "not enough packed bytes")
    out = np.empty(max(n, 1), dtype=np.uint8)
    rc = load_library().demod_unpack_symbols(_ptr(src), n, bits, _ptr(out), n)
    if rc < 0:
        raise DemodError(rc, "demod_unpack_symbols")
    return out[:n]


def frame_symbols(symbols: np.ndarray, bits: int,
                  max_payload: int = DEMOD_MAX_FRAME_PAYLOAD) -> bytes:
    """Symbols -> consecutive delimited ToReceiver frames (rank-0 framing)."""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    per = max_payload * 8 // bits
    nframes = (sym.size + per - 1) // per
    cap = nframes * frame_size(max_payload) + 16
    out = np.empty(cap, dtype=np.uint8)
    rc = load_library().demod_frame_symbols(_ptr(sym), sym.size, bits, max_payload,
                                            _ptr(out), cap)
    if rc < 0:
        raise DemodError(int(rc), "demod_frame_symbols")
    return out[:rc].tobytes()


def frame_symbols_size(n: int, bits: int, max_payload: int = DEMOD_MAX_FRAME_PAYLOAD) -> int:
    """Bytes frame_symbols produces for n symbols."""
    rc = int(load_library().demod_frame_symbols_size(n, bits, max_payload))
    if rc < 0:
        raise DemodError(rc, "demod_frame_symbols_size")
    return rc


def frame_streams_async(d_symbols, n_streams: int, n: int, bits: int, d_out,
                        max_payload: int = DEMOD_MAX_FRAME_PAYLOAD, stream: int = 0) -> int:
    """Device framing of [n_streams][n] symbols: stream s's frames (as
    frame_symbols would make them) at d_out[s * stride]; returns stride."""
    stride = frame_symbols_size(n, bits, max_payload)
    _check_dev(d_symbols, "d_symbols", "uint8", int(n_streams) * int(n))
    _check_dev(d_out, "d_out", "uint8", int(n_streams) * stride)
    if d_symbols is not None and d_out is not None and d_symbols.device != d_out.device:
        raise DemodError(DEMOD_BAD_ARG, "d_symbols and d_out on different devices")
    rc = int(load_library().demod_frame_streams_async(_ptr(d_symbols), n_streams, n, bits,
                                                      max_payload, _ptr(d_out), stream or None))
    if rc < 0:
        raise DemodError(rc, "demod_frame_streams_async")
    return rc


def iter_frames(stream: bytes):
    """Yield payloads of consecutive delimited frames (network.cpp:409-430 loop)."""
    pos = 0
    while pos < len(stream):
        payload, used = frame_decode(stream[pos:])
        yield payload
        pos += used


# ---- many streams over many GPUs (demod_group_*, RCCL) -----------------------

DEMOD_GROUP_ID_BYTES = 128


def group_unique_id() -> bytes:
    """demod_group_unique_id: a fresh RCCL group id (rank 0 shares it)."""
    buf = (ctypes.c_uint8 * DEMOD_GROUP_ID_BYTES)()
    rc = load_library().demod_group_unique_id(buf)
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_group_unique_id")
    return bytes(buf)


def group_shard(n_streams: int, rank: int, world: int) -> Tuple[int, int]:
    f, c = _SZ(), _SZ()
    rc = load_library().demod_group_shard(n_streams, rank, world, ctypes.byref(f), ctypes.byref(c))
    if rc != DEMOD_OK:
        raise DemodError(rc, "demod_group_shard")
    return f.value, c.value


def group_block_bytes(n_streams: int, world: int, steps: int, symbols_per_stream: int, bits: int) -> int:
    rc = load_library().demod_group_block_bytes(n_streams, world, steps, symbols_per_stream, bits)
    if rc < 0:
        raise DemodError(int(rc), "demod_group_block_bytes")
    return int(rc)


class Group(_Handle):
    """demod_group_t: n_streams streams sharded over `world` GPUs, RCCL gathers.
    Group(cfg, n, rank=r, world=w, uid=...) is one rank of a multi-process
    group; Group(cfg, n, devices=[...]) drives every rank in this process."""
    _destroy = "demod_group_destroy"

    def __init__(self, cfg: DemodCfg, n_streams: int, rank: int = 0, world: int = 1,
                 uid: Optional[bytes] = None, devices: Optional[Sequence[int]] = None):
        self._lib = load_library()
        err = ctypes.c_int(0)
        if devices is not None:
            arr = (ctypes.c_int * len(devices))(*devices)
            self._h = self._lib.demod_group_create_local(ctypes.byref(cfg), n_streams, len(devices), arr,
                                                         ctypes.byref(err))
        else:
            if uid is None:
                uid = group_unique_id()
            buf = (ctypes.c_uint8 * DEMOD_GROUP_ID_BYTES).from_buffer_copy(uid)
            self._h = self._lib.demod_group_create(ctypes.byref(cfg), n_streams, rank, world, buf,
                                                   ctypes.byref(err))
        if not self._h:
            raise DemodError(err.value, "demod_group_create")
        self.n_streams = n_streams
        self.k = cfg.k
        self.channels = int(cfg.channels)
        self.world = self._lib.demod_group_world(self._h)
        self.local_ranks = self._lib.demod_group_local_ranks(self._h)

    def shard(self, local: int = 0) -> Tuple[int, int, int]:
        """(rank, first stream, count) of the local-th rank this process drives."""
        r, f, c = ctypes.c_int(), _SZ(), _SZ()
        rc = self._lib.demod_group_rank_shard(self._h, local, ctypes.byref(r), ctypes.byref(f),
                                              ctypes.byref(c))
        if rc != DEMOD_OK:
            raise DemodError(rc, "demod_group_rank_shard")
        return r.value, f.value, c.value

    def device(self, local: int = 0) -> int:
        """demod_group_rank_device: the GPU of the local-th rank this process drives."""
        rc = self._lib.demod_group_rank_device(self._h, local)
        if rc < 0:
            raise DemodError(rc, "demod_group_rank_device")
        return rc

    def status(self) -> int:
        """demod_group_status: DEMOD_OK while alive, else the code that killed it."""
        return self._lib.demod_group_status(self._h)

    def wait(self, streams: Optional[Sequence[int]] = None) -> None:
        """demod_group_wait: wait for the last bucket on `streams`; raises the
        lowest failing rank's code (the same on every rank)."""
        n = self.local_ranks
        ps = (ctypes.c_void_p * n)(*(streams or [0] * n))
        rc = self._lib.demod_group_wait(self._h, ps if streams else None)
        if rc != DEMOD_OK:
            raise DemodError(rc, "demod_group_wait")

    def push(self, packets: Sequence[np.ndarray], cap: Optional[int] = None):
        """One packet per stream this process owns -> (symbols of every stream,
        counts per stream)."""
        packets = [np.ascontiguousarray(p, dtype=np.int16) for p in packets]
        nf = (_SZ * len(packets))(*[p.size // self.channels for p in packets])
        ptrs = (ctypes.c_void_p * len(packets))(*[p.ctypes.data if p.size else None for p in packets])
        if cap is None:
            cap = sum(p.size for p in packets) * max(self.world, 1) + 64 * self.n_streams
        sym = np.zeros(max(cap, 1), np.uint8)
        counts = np.zeros(self.n_streams, np.uint32)
        rc = self._lib.demod_group_push(self._h, ptrs, nf, sym.ctypes.data, cap, counts.ctypes.data)
        if rc < 0:
            raise DemodError(rc, "demod_group_push")
        return sym[:rc], counts

    def bucket_async(self, d_pcm: Sequence, ring: int, wps: int, steps: int, d_all: Sequence,
                     streams: Optional[Sequence[int]] = None) -> int:
        """demod_group_bucket_async over the ranks this process drives."""
        n = len(d_all)
        pc = (ctypes.c_void_p * n)(*[_ptr(t) for t in d_pcm])
        pa = (ctypes.c_void_p * n)(*[_ptr(t) for t in d_all])
        ps = (ctypes.c_void_p * n)(*(streams or [0] * n))
        rc = self._lib.demod_group_bucket_async(self._h, pc, ring, wps, steps, pa, ps)
        if rc < 0:
            raise DemodError(int(rc), "demod_group_bucket_async")
        return int(rc)
