"""ctypes binding of libtinyvc_hip.so (the C ABI in include/tinyvc_hip.h).

There is no fallback: if the shared library is missing or a call fails, this raises.  The
library is built in-tree by `tinyvc_amd.build.build()` (hipcc, gfx950).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TVC_LIB_PATH") or os.path.join(_HERE, "libtinyvc_hip.so")   # TVC_LIB_PATH: same-box A/B runs of two builds

_lib = None


class PitchPathSettings(ctypes.Structure):
    """tvc_pitch_path of include/tinyvc_hip.h: the host settings of the pitch path"""
    _fields_ = [("step", c_float), ("band", c_int32), ("jump", c_float), ("voicing", c_float), ("refine", c_int32)]


class PitchSnapSettings(ctypes.Structure):
    """tvc_pitch_snap of include/tinyvc_hip.h: the host settings of the pitch correction"""
    _fields_ = [("hysteresis", c_float), ("retune", c_float), ("f_min", c_float), ("f_max", c_float)]


PTR, INT, I64, F32, U64, SIZE, STR = c_void_p, c_int, c_int64, c_float, c_uint64, c_size_t, c_char_p
PTRS, INTS, I64S, F32S, SIZES, PATH = POINTER(c_void_p), POINTER(c_int), POINTER(c_int64), POINTER(c_float), POINTER(c_size_t), POINTER(PitchPathSettings)
SNAP_SETTINGS = POINTER(PitchSnapSettings)


def _fn(restype, *groups, **params):
    """(restype, ((parameter name, ctype), ...)): the groups (dicts) in order, then the keywords; a name that comes twice is an error"""
    out = {}
    for g in groups + (params,):
        if out.keys() & g.keys():
            raise TypeError(f"parameter declared twice: {sorted(out.keys() & g.keys())}")
        out.update(g)
    return restype, tuple(out.items())


# The conversion ladder's parameters, by the groups the header's prototypes are made of: every rung is the one below it plus a group.
CALL = dict(ctx=PTR, stream=PTR)
SHARED = dict(prepared_index=PTR, N=I64)      # one index for every row; the stage call (tvc_knn_match_f32) says `prepared`
TABLE = dict(prepared=PTRS, N=I64S)           # host tables, one entry per row
BLEND = dict(TABLE, M=INT, weights=PTR)       # ... M per row, and the device weights (NULL with M = 1: the table call)
ALPHA, PROTECT, PITCH_PATH, CARRY, TARGET = dict(alpha=PTR), dict(protect=PTR), dict(path=PATH), dict(carry_frame=INT, carry=PTR), dict(target_f0=PTR)
WEIGHTED = dict(neighbours=PTR, width=PTR)      # the weighted match: k (int32) and the similarity width (fp32) per row, on the device
JOINED = dict(WEIGHTED, join=PTR)               # ... and the continuity weight (fp32) per row of the match along a path, on the device
SNAP = dict(snap=SNAP_SETTINGS, notes=PTR, strength=PTR)      # the pitch correction: host settings, the table and the strengths on the device
SNAP_STATE = dict(snap_carry_frame=INT, snap_note=PTR, snap_ratio=PTR)
TRACK = dict(start=INT, n=INT, W=INT, min_voiced=INT, slew=F32, ring=PTR, count=PTR, auto_shift=PTR)
SHIFT = dict(pitch_shift=F32)
SHIFTS = dict(SHIFT, pitch_shifts=F32S)
SHIFTS_OUT = dict(SHIFTS, shift_out=PTR)
NOISE = dict(noise_angle=PTR, seed=U64, wave=PTR)
WS = dict(ws=PTR, ws_bytes=SIZE)
EQUAL, RAGGED = (dict(wav=PTR), dict(B=INT, L=I64, **WS)), (dict(wav=PTR, Lmax=I64, lens=I64S), dict(B=INT, **WS))      # (head, tail) of a conversion
Q_EQUAL, Q_RAGGED = dict(ctx=PTR, B=INT, L=I64), dict(ctx=PTR, B=INT, Lmax=I64, lens=I64S)                                # the head of its query
MATCH = dict(out=PTR, idx_out=PTR, B=INT, T=INT, **WS)                                                                     # the tail of a match


def _convert(rows, *groups):
    return _fn(INT, CALL, rows[0], *groups, NOISE, rows[1])


def _query(head, **index):
    return _fn(INT, head, index, out_bytes=SIZES)


_BLEND_Q = dict(N=I64S, M=INT)

# name -> (restype, ((parameter name, ctype), ...)); mirrors include/tinyvc_hip.h one to one, names included (tests/test_cabi.py)
PROTOTYPES = {
    "tvc_version": _fn(INT),
    "tvc_ctx_create": _fn(INT, hip_device=INT, out=PTRS),
    "tvc_ctx_destroy": _fn(None, ctx=PTR),
    "tvc_last_error": _fn(STR, ctx=PTR),
    "tvc_load_tensor": _fn(INT, ctx=PTR, state_dict_key=STR, host_data=PTR, shape=I64S, ndim=INT),
    "tvc_set_pitch_table": _fn(INT, ctx=PTR, host_freqs=PTR, n=INT),
    "tvc_finalize_weights": _fn(INT, ctx=PTR),
    "tvc_stft_mag_f32": _fn(INT, CALL, wav=PTR, spec=PTR, B=INT, L=I64, **WS),
    "tvc_energy_f32": _fn(INT, CALL, wav=PTR, energy=PTR, B=INT, L=I64, **WS),
    "tvc_resample_out_len": _fn(I64, n=I64, orig_freq=INT, new_freq=INT),
    "tvc_resample_f32": _fn(INT, CALL, x=PTR, y=PTR, rows=INT, n=I64, orig_freq=INT, new_freq=INT),
    "tvc_pcm16_to_f32": _fn(INT, CALL, pcm=PTR, y=PTR, n=I64, gain_db=F32),
    "tvc_f32_to_pcm16": _fn(INT, CALL, x=PTR, pcm=PTR, n=I64, gain_db=F32),
    "tvc_encoder_f32": _fn(INT, CALL, spec=PTR, ssl=PTR, f0=PTR, logits=PTR, B=INT, T=INT, **WS),
    "tvc_pitch_decode_f32": _fn(INT, CALL, logits=PTR, f0=PTR, B=INT, T=INT),
    "tvc_knn_prepared_elems": _fn(I64, N=I64),
    "tvc_knn_prepared_elems_f16": _fn(I64, N=I64),
    "tvc_knn_prepare_index_f32": _fn(INT, CALL, index=PTR, prepared=PTR, N=I64),
    "tvc_knn_prepare_index_f16": _fn(INT, CALL, rows_f16=PTR, prepared=PTR, N=I64),
    "tvc_knn_prepare_index_cols_f32": _fn(INT, CALL, feats=PTR, S=I64, cols=PTR, N=I64, prepared=PTR, index_out=PTR),
    "tvc_knn_prepare_index_cols_f16": _fn(INT, CALL, feats=PTR, S=I64, cols=PTR, N=I64, prepared=PTR, index_out_f16=PTR),
    "tvc_knn_forget": _fn(INT, ctx=PTR, prepared=PTR),
    "tvc_ragged_plan": _fn(INT, B=INT, Lmax=I64, lens=I64S, max_frames=INT, batch_of_row=POINTER(c_int32), n_batches=INTS),
    "tvc_ctx_set_ragged_batch_frames": _fn(INT, ctx=PTR, max_frames=INT),
    "tvc_knn_match_general_f32": _fn(INT, CALL, src=PTR, index=PTR, N=I64, k=INT, metric=INT, out=PTR, idx_out=PTR, sim_out=PTR, B=INT, T=INT, **WS),
    "tvc_knn_topk_f32": _fn(INT, CALL, src=PTR, prepared=PTR, N=I64, sims_out=PTR, idx_out=PTR, B=INT, T=INT, **WS),
    "tvc_knn_gather_slots_f32": _fn(INT, CALL, prepared=PTR, N=I64, idx=PTR, slots=PTR, nslots=I64),
    "tvc_knn_finish_f32": _fn(INT, CALL, slots=PTR, out=PTR, B=INT, T=INT),
    "tvc_shift_frequency_f32": _fn(INT, CALL, f0=PTR, out=PTR, n=I64, semitones=F32),
    "tvc_noise_angle_from_uniform_f32": _fn(INT, CALL, u=PTR, n=I64),
    "tvc_decoder_f32": _fn(INT, CALL, content=PTR, f0=PTR, energy=PTR, noise_angle=PTR, seed=U64, wave=PTR, B=INT, T=INT, **WS),
    "tvc_decoder_stages_f32": _fn(INT, CALL, content=PTR, f0=PTR, energy=PTR, noise_angle=PTR, seed=U64, wave=PTR, amps=PTR, kernel=PTR, source=PTR, B=INT, T=INT, **WS),
    "tvc_filter_net_f32": _fn(INT, CALL, content=PTR, f0=PTR, energy=PTR, source=PTR, wave=PTR, skips=PTRS, ups=PTRS, B=INT, T=INT, **WS),
    "tvc_dsp_f32": _fn(INT, CALL, f0=PTR, amps=PTR, kernel=PTR, noise_angle=PTR, seed=U64, source=PTR, B=INT, T=INT, **WS),
    "tvc_workspace_bytes_encode_ragged": _fn(INT, Q_RAGGED, out_bytes=SIZES),
    "tvc_encode_ragged_f32": _fn(INT, CALL, RAGGED[0], dict(ssl=PTR, f0=PTR), RAGGED[1]),
    # ---- the ladder: 16 conversions, their 14 workspace queries, 5 matches
    "tvc_workspace_bytes": _query(Q_EQUAL, N=I64),
    "tvc_workspace_bytes_ragged": _query(Q_RAGGED, N=I64),
    "tvc_workspace_bytes_multi": _query(Q_EQUAL, N=I64S),
    "tvc_workspace_bytes_ragged_multi": _query(Q_RAGGED, N=I64S),
    "tvc_workspace_bytes_blend": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_blend": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_workspace_bytes_auto": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_auto": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_workspace_bytes_alpha": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_alpha": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_workspace_bytes_protect": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_protect": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_workspace_bytes_path": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_path": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_convert_f32": _convert(EQUAL, SHARED, SHIFT),
    "tvc_convert_ragged_f32": _convert(RAGGED, SHARED, SHIFT),
    "tvc_convert_multi_f32": _convert(EQUAL, TABLE, SHIFTS),
    "tvc_convert_ragged_multi_f32": _convert(RAGGED, TABLE, SHIFTS),
    "tvc_convert_blend_f32": _convert(EQUAL, BLEND, SHIFTS),
    "tvc_convert_ragged_blend_f32": _convert(RAGGED, BLEND, SHIFTS),
    "tvc_convert_auto_f32": _convert(EQUAL, BLEND, TARGET, SHIFTS_OUT),
    "tvc_convert_ragged_auto_f32": _convert(RAGGED, BLEND, TARGET, SHIFTS_OUT),
    "tvc_convert_track_f32": _convert(EQUAL, BLEND, TARGET, TRACK, SHIFTS_OUT),      # streams advance in lock step: a tracker or a carry has no ragged form
    "tvc_convert_alpha_f32": _convert(EQUAL, BLEND, ALPHA, TARGET, TRACK, SHIFTS_OUT),
    "tvc_convert_ragged_alpha_f32": _convert(RAGGED, BLEND, ALPHA, TARGET, SHIFTS_OUT),
    "tvc_convert_protect_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, TARGET, TRACK, SHIFTS_OUT),
    "tvc_convert_ragged_protect_f32": _convert(RAGGED, BLEND, ALPHA, PROTECT, TARGET, SHIFTS_OUT),
    "tvc_convert_path_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, PITCH_PATH, TARGET, TRACK, SHIFTS_OUT),
    "tvc_convert_ragged_path_f32": _convert(RAGGED, BLEND, ALPHA, PROTECT, PITCH_PATH, TARGET, SHIFTS_OUT),
    "tvc_convert_carry_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, PITCH_PATH, CARRY, TARGET, TRACK, SHIFTS_OUT),
    # the tuned entries: the carry call / the ragged path call with the correction in front of the decoder (not rungs of the ladder: snap == NULL is the sibling)
    "tvc_tuned_convert_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, PITCH_PATH, CARRY, SNAP, SNAP_STATE, TARGET, TRACK, SHIFTS_OUT),
    "tvc_tuned_convert_ragged_f32": _convert(RAGGED, BLEND, ALPHA, PROTECT, PITCH_PATH, SNAP, TARGET, SHIFTS_OUT),
    # the weighted entries: the tuned entries / the protect match with k and the similarity width behind protect (both NULL: the sibling)
    "tvc_weighted_convert_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, WEIGHTED, PITCH_PATH, CARRY, SNAP, SNAP_STATE, TARGET, TRACK, SHIFTS_OUT),
    "tvc_weighted_convert_ragged_f32": _convert(RAGGED, BLEND, ALPHA, PROTECT, WEIGHTED, PITCH_PATH, SNAP, TARGET, SHIFTS_OUT),
    "tvc_knn_match_weighted_f32": _fn(INT, CALL, dict(src=PTR, f0=PTR), BLEND, ALPHA, PROTECT, WEIGHTED,
                                      dict(out=PTR, idx_out=PTR, sims_out=PTR, B=INT, T=INT, **WS)),
    # the joined entries: the weighted entries with the continuity weight behind width (NULL: the sibling), the path's outputs behind sims_out
    "tvc_workspace_bytes_joined": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_workspace_bytes_ragged_joined": _query(Q_RAGGED, **_BLEND_Q),
    "tvc_workspace_bytes_match_joined": _query(Q_EQUAL, **_BLEND_Q),
    "tvc_joined_convert_f32": _convert(EQUAL, BLEND, ALPHA, PROTECT, JOINED, PITCH_PATH, CARRY, SNAP, SNAP_STATE, TARGET, TRACK, SHIFTS_OUT),
    "tvc_joined_convert_ragged_f32": _convert(RAGGED, BLEND, ALPHA, PROTECT, JOINED, PITCH_PATH, SNAP, TARGET, SHIFTS_OUT),
    "tvc_knn_match_joined_f32": _fn(INT, CALL, dict(src=PTR, f0=PTR), BLEND, ALPHA, PROTECT, JOINED,
                                    dict(out=PTR, idx_out=PTR, sims_out=PTR, anchor_out=PTR, affinity_out=PTR, B=INT, T=INT, **WS)),
    "tvc_knn_match_f32": _fn(INT, CALL, dict(src=PTR, prepared=PTR, N=I64), MATCH),
    "tvc_knn_match_multi_f32": _fn(INT, CALL, dict(src=PTR), TABLE, MATCH),
    "tvc_knn_match_blend_f32": _fn(INT, CALL, dict(src=PTR), BLEND, MATCH),
    "tvc_knn_match_alpha_f32": _fn(INT, CALL, dict(src=PTR), BLEND, ALPHA, MATCH),
    "tvc_knn_match_protect_f32": _fn(INT, CALL, dict(src=PTR, f0=PTR), BLEND, ALPHA, PROTECT, MATCH),
    # ---- the pitch stage calls
    "tvc_pitch_match_f32": _fn(INT, CALL, dict(f0=PTR, row_start=I64S, rows=INT), TARGET, SHIFTS, median_out=PTR, voiced_out=PTR, shift_out=PTR, f0_shifted=PTR),
    "tvc_pitch_track_f32": _fn(INT, CALL, dict(f0=PTR, S=INT, T=INT, start=INT, n=INT), TARGET, SHIFTS, W=INT, min_voiced=INT, slew=F32, ring=PTR, count=PTR,
                               auto_shift=PTR, median_out=PTR, count_out=PTR, shift_out=PTR, f0_shifted=PTR),
    "tvc_frame_share_f32": _fn(INT, CALL, dict(f0=PTR, row_start=I64S, row_count=I64S, rows=INT), ALPHA, PROTECT, share_out=PTR),
    "tvc_workspace_bytes_pitch_path": _fn(INT, ctx=PTR, row_start=I64S, row_count=I64S, rows=INT, out_bytes=SIZES),
    "tvc_pitch_path_f32": _fn(INT, CALL, dict(logits=PTR, row_start=I64S, row_count=I64S, rows=INT, class_stride=I64), PITCH_PATH, SHIFTS, f0=PTR, f0_shifted=PTR,
                              path_out=PTR, score_out=PTR, **WS),
    "tvc_pitch_path_carry_f32": _fn(INT, CALL, dict(logits=PTR, row_start=I64S, row_count=I64S, rows=INT, class_stride=I64), PITCH_PATH,
                                    dict(carry_frame=INT, prior=PTR, carry_out=PTR), SHIFTS, f0=PTR, f0_shifted=PTR, path_out=PTR, score_out=PTR, **WS),
    "tvc_pitch_snap_f32": _fn(INT, CALL, dict(f0=PTR, row_start=I64S, row_count=I64S, rows=INT), SNAP, carry_frame=INT, note=PTR, ratio=PTR, out=PTR, note_out=PTR),
    # ---- index compaction
    "tvc_ctx_set_index_assign_chunk": _fn(INT, ctx=PTR, max_queries=INT),
    "tvc_workspace_bytes_index_compact": _fn(INT, ctx=PTR, N=I64, K=I64, out_bytes=SIZES),
    "tvc_index_assign_f32": _fn(INT, CALL, points_prepared=PTR, N=I64, centroids_prepared=PTR, K=I64, assign_inout=PTR, sim_out=PTR, moved_out=PTR, **WS),
    "tvc_index_update_f32": _fn(INT, CALL, points_prepared=PTR, N=I64, assign=PTR, K=I64, centroids_inout=PTR, counts_out=PTR, **WS),
    "tvc_index_compact_f32": _fn(INT, CALL, points_prepared=PTR, N=I64, init_cols=PTR, K=I64, iters=INT, centroids_out=PTR, prepared_out=PTR, assign_out=PTR,
                                 counts_out=PTR, moved_out=PTR, **WS),
    # ---- the stream stages
    "tvc_sola_f32": _fn(INT, CALL, y=PTR, sola_buf=PTR, fade_in=PTR, out=PTR, shift_out=PTR, S=INT, Ly=I64, block=INT, use_phase_vocoder=INT),
    "tvc_sola_geom_f32": _fn(INT, CALL, y=PTR, sola_buf=PTR, fade_in=PTR, out=PTR, shift_out=PTR, S=INT, Ly=I64, block=INT, cross=INT, search=INT, delay=INT,
                             use_phase_vocoder=INT),
    "tvc_sola_geometry": _fn(INT, block=INT, cross=INT, search=INT, delay=INT, min_ly=I64S, latency_min=INTS, latency_max=INTS),
    "tvc_sola_geometry_message": _fn(STR, block=INT, cross=INT, search=INT, delay=INT),
    "tvc_stream_push_f32": _fn(INT, CALL, buf=PTR, blocks=PTR, S=INT, n=I64, block=INT),
    "tvc_stream_resample_geometry": _fn(INT, in_freq=INT, out_freq=INT, n_in=I64, n_out=I64S, hist=INTS, delay=INTS),
    "tvc_stream_resample_prepare": _fn(INT, ctx=PTR, in_freq=INT, out_freq=INT),
    "tvc_stream_resample": _fn(INT, CALL, {"in": PTR}, in_is_pcm16=INT, out=PTR, out_is_pcm16=INT, state=PTR, S=INT, n_in=I64, in_freq=INT, out_freq=INT, gain_db=F32),
    "tvc_stream_gate_geometry": _fn(INT, block=INT, sub=INT, look=INT, hold=INT, attack=INT, release=INT, nsub=INTS, look_samples=INTS),
    "tvc_stream_gate_geometry_message": _fn(STR, block=INT, sub=INT, look=INT, hold=INT, attack=INT, release=INT),
    "tvc_stream_gate_f32": _fn(INT, CALL, x=PTR, n=I64, base=I64, shift=PTR, y=PTR, out=PTR, S=INT, block=INT, sub=INT, look=INT, hold=INT, attack=INT, release=INT,
                               hysteresis_db=F32, range_db=F32, threshold_db=PTR, open=PTR, hold_state=PTR, gain=PTR, level_db=PTR),
    "tvc_stream_denoise_geometry": _fn(INT, block=INT, hop=INT, frames=INTS, delay=INTS),
    "tvc_stream_denoise_geometry_message": _fn(STR, block=INT, hop=INT),
    "tvc_stream_denoise_f32": _fn(INT, CALL, x=PTR, out=PTR, S=INT, block=INT, hop=INT, a_s=F32, a_n=F32, clamp=F32, beta=F32, warm=INT, reduction_db=PTR, hist=PTR,
                                  ola=PTR, smooth=PTR, noise=PTR, frames=PTR, noise_db=PTR),
    "tvc_loudness_geometry": _fn(INT, length=I64, sub=INT, smooth=INT, nsub=I64S, window=INTS, tile=INTS),
    "tvc_loudness_geometry_message": _fn(STR, length=I64, sub=INT, smooth=INT),
    "tvc_stream_loudness_geometry": _fn(INT, block=INT, sub=INT, smooth=INT, nsub=INTS, window=INTS),
    "tvc_stream_loudness_geometry_message": _fn(STR, block=INT, sub=INT, smooth=INT),
    "tvc_loudness_match_f32": _fn(INT, CALL, x=PTR, y=PTR, out=PTR, B=INT, L=I64, lengths=I64S, share=PTR, sub=INT, smooth=INT, floor_db=F32, boost_db=F32, cut_db=F32,
                                  gains=PTR),
    "tvc_stream_loudness_f32": _fn(INT, CALL, x=PTR, n=I64, base=I64, shift=PTR, y=PTR, out=PTR, S=INT, block=INT, sub=INT, smooth=INT, floor_db=F32, boost_db=F32,
                                   cut_db=F32, share=PTR, src_ring=PTR, out_ring=PTR, frames=PTR, gain=PTR, gain_db=PTR, gains=PTR),
    "tvc_limiter_geometry": _fn(INT, length=I64, sub=INT, release=INT, nsub=I64S, delay=INTS, tile=INTS),
    "tvc_limiter_geometry_message": _fn(STR, length=I64, sub=INT, release=INT),
    "tvc_stream_limiter_geometry": _fn(INT, block=INT, sub=INT, release=INT, nsub=INTS, delay=INTS, chunk=INTS),
    "tvc_stream_limiter_geometry_message": _fn(STR, block=INT, sub=INT, release=INT),
    "tvc_limit_f32": _fn(INT, CALL, y=PTR, out=PTR, B=INT, L=I64, lengths=I64S, ceiling=PTR, sub=INT, release=INT, drive_db=F32, gains=PTR),
    "tvc_stream_limit_f32": _fn(INT, CALL, y=PTR, out=PTR, S=INT, block=INT, sub=INT, release=INT, drive_db=F32, ceiling=PTR, tail=PTR, peak=PTR, gain=PTR,
                                reduction_db=PTR, gains=PTR),
    "tvc_profile_enable": _fn(INT, ctx=PTR, on=INT),
    "tvc_profile_read": _fn(INT, ctx=PTR, buf=STR, buf_bytes=SIZE),
}
# name -> (restype, [argtypes]): what load_library declares
SIGNATURES = {name: (res, [t for _n, t in params]) for name, (res, params) in PROTOTYPES.items()}
_NAMES = {name: tuple(n for n, _t in params) for name, (_res, params) in PROTOTYPES.items()}
_NAMESET = {name: frozenset(names) for name, names in _NAMES.items()}


def arguments(entry, named):
    """The values of `named` (parameter name -> value) in the order `entry` declares its parameters.  TypeError for a declared
    parameter without a value, and for a value the entry has no parameter for unless it is "off" (None, 0, 0.0): nothing is dropped or
    moved by a slot in silence."""
    names = _NAMES[entry]
    try:
        args = tuple([named[n] for n in names])
    except KeyError as e:
        raise TypeError(f"{entry}: no value for its parameter `{e.args[0]}`") from None
    if len(named) > len(names):
        declared = _NAMESET[entry]
        for k, v in named.items():
            if v is not None and k not in declared and not (isinstance(v, (int, float)) and v == 0):
                raise TypeError(f"{entry} has no parameter `{k}`, and its value {v!r} is not \"off\" (None, 0, 0.0)")
    return args


class TinyVCError(RuntimeError):
    pass


def load_library():
    """Load libtinyvc_hip.so and declare every prototype.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles the HIP runtime (SONAME libamdhip64.so.7) and must be the one copy
    # in the process; loaded after our .so it would come in as a second runtime next to /opt/rocm's.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise TinyVCError(
            f"{LIB_PATH} is missing: build it with `python -m tinyvc_amd.build` (needs hipcc). "
            "tinyvc_amd has no CPU or eager-PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
