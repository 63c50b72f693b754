"""Generator = encoder -> kNN match -> pitch shift -> decoder (reference module/infer/generator.py:12-34): whatever form the target takes,
`convert` is one host path that ends in one call of the tvc_convert*_f32 entry that form belongs to (Engine._convert)."""
import torch

from .. import utils
from ...engine import loudness_in_place, pitch_shifts
from .._base import HipModule
from ..tinyvc import Decoder, Encoder
from ..tinyvc.feature_retrieval import (alpha_rows, continuity_rows, resolve_continuity, match_k_rows, match_width_rows, resolve_match_k, resolve_match_width, check_blend, check_references, check_tune_carry, resolve_tune, limit_rows, loudness_rows, prepare_reference, prepare_references,
                                        protect_rows, resolve_alpha, resolve_auto_pitch, resolve_f0_estimation, resolve_limit, resolve_loudness,
                                        resolve_protect, target_form, target_registers)


def _padded_lengths(lengths, B, L):
    """a ragged batch's lengths, each rounded up to whole frames: one per row, each in (960, L]"""
    lens = [-(-int(n) // 480) * 480 for n in lengths]
    if len(lens) != B or max(lens) > L or min(lens) <= 960:
        raise ValueError("lengths: one entry per row, each in (960, L]")
    return lens


class Generator(HipModule):
    def __init__(self, encoder: Encoder, decoder: Decoder):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder

    def _weight_tensors(self):
        sd = dict(self.encoder.state_dict())
        sd.update(self.decoder.state_dict())
        return sd

    @torch.no_grad()
    def encode(self, wf, lengths=None):
        """generator.py:19-23: wf [B, L] -> (features [B,768,T] usable as a kNN index, f0 [B,1,T]).
        `lengths` (extension): a RAGGED batch - row b of wf holds a clip of lengths[b] samples, zero-padded behind it.  Every clip is
        encoded over its own length (padded to a multiple of 480) in one call and equals its own `encode` bit for bit; the result is
        (list of B [1, 768, T_b] views of ONE packed [768, sum T_b] tensor, list of B [1, 1, T_b])."""
        if lengths is None:
            wf = utils.autopad_waveform(self._input_device(wf))
            eng = self.engine(wf.device)
            ssl, f0, _ = eng.encoder(eng.stft_mag(wf))
            return ssl, f0
        ssl, f0, pre = self.encode_packed(wf, lengths)
        return ([ssl[None, :, pre[b]:pre[b + 1]] for b in range(len(pre) - 1)],
                [f0[None, None, pre[b]:pre[b + 1]] for b in range(len(pre) - 1)])

    @torch.no_grad()
    def encode_packed(self, wf, lengths):
        """The ragged `encode` as it leaves the device: (features [768, S], f0 [S], pre [B + 1]) - clip b owns columns pre[b] .. pre[b + 1]
        (Engine.encode_ragged); what build_index selects its columns from."""
        wf = utils.autopad_waveform(self._input_device(wf))
        B, L = wf.shape
        return self.engine(wf.device).encode_ragged(wf, _padded_lengths(lengths, B, L))

    @torch.no_grad()
    def convert(self, wf, tgt, pitch_shift, f0_estimation="default", device=None, noise_angle=None, lengths=None, auto_pitch=None,
                return_shift=False, track=None, alpha=None, protect=None, loudness=None, limit=None, carry=None, tune=None, tune_carry=None, k=None,
                match_width=None, continuity=None):
        """generator.py:26-34: wf [B, L], tgt [1 or B, 768, N] -> converted waveform [B, L'] (L' = L
        padded to a multiple of 480).  `f0_estimation` / `device` are accepted and ignored exactly as
        in the reference - but for `f0_estimation='viterbi'` or a feature_retrieval.PitchPath (extension): f0 is then the pitch path, a
        Viterbi decode of the call's own pitch logits over each utterance as a whole (a ragged batch: each utterance's own frames) in the place
        of the per-frame top-4 expectation, inside the same call (tvc_convert_path_f32 / tvc_convert_ragged_path_f32: one more launch directly
        behind the encoder), and protect's voicing, auto_pitch, track, the shift and the decoder read that f0.  Every target form, equal and
        ragged, with every other keyword.  'viterbi' is PitchPath() with its defaults, which are guesses: nobody has listened.  `noise_angle` [B,961,T] (extension) injects the decoder's noise phases;
        by default the library draws them itself (seeded from torch's generator: Decoder.draw_noise_angle).
        `lengths` (extension): a RAGGED batch - row b of wf holds an utterance of lengths[b] samples, zero-padded behind it.
        Every utterance is converted over its own length (padded to a multiple of 480), exactly as if it were converted
        alone (the reference's loop, infer.py:60-66; GRN and the oscillator's phase run over the whole time axis, so padding
        to a common length would change the results); row b of the result holds it, zeros behind.
        One index per row: tgt [B, 768, N] (the reference's form) or a list of B [1, 768, N_b] tensors (extension: fp32 or fp16,
        any N_b), equal or ragged batches, in one call (tvc_convert_multi_f32 / tvc_convert_ragged_multi_f32: row b equals its own
        B = 1 conversion against tgt[b]).  `pitch_shift` (extension): a float, or a sequence / 1-D tensor of one shift per row.
        A weighted blend of indices (extension): tgt = feature_retrieval.Blend(terms, weights) converts every frame toward
        w_0 * match_0 + w_1 * match_1 + ... in ONE call (tvc_convert_blend_f32 / tvc_convert_ragged_blend_f32), equal or ragged batches,
        scalar or per-row shifts; the weights are read on the device when the kernels run.
        `auto_pitch` (extension): move every row's median f0 onto the target's register, on the device inside the same call
        (tvc_convert_auto_f32 / tvc_convert_ragged_auto_f32: no second encoder pass, no host synchronisation) - a register in Hz (a float, or
        a [B] / [1] device tensor, read when the kernels run), or True = the register riding on each target tensor (`pitch_register`:
        build_index and the entry scripts' loaders attach it).  True is refused (ValueError, before any engine work) for a target without a
        register and for a Blend, which takes an explicit register.  `pitch_shift` then is the offset on top of the automatic shift.
        `return_shift=True` -> (wave, shifts [B] on the device: the semitones applied to each row).
        `track` (extension, with auto_pitch): a feature_retrieval.PitchTrack of B streams - the register each row is moved FROM is then the
        lower median of the stream's history (the tracker's ring on the device, fed by columns [T - lag_frames - new_frames, T - lag_frames)
        of this call's f0), slew-limited, instead of the median of the call's own rows (tvc_convert_track_f32; equal lengths only).
        `alpha` (extension; the reference's match_features(..., alpha), which its convert never passes): keep that share of every row's own
        content features - matched * (1 - alpha) + features * alpha, inside the same call (tvc_convert_alpha_f32 /
        tvc_convert_ragged_alpha_f32) - a float, a list of B floats, or an fp32 [B] / [1] device tensor ([B]: used in place, read when the
        kernels run).  Every target form, equal and ragged batches, with auto_pitch and track.  None (the default) is the call without it.
        `protect` (extension; RVC's protect, as 1 - its value): raise that share on UNVOICED frames only - frame t keeps
        a_t = alpha + (1 - alpha) * (protect * w[t]) of its own features, w[t] = 1 - (u[t-1] + 2 u[t] + u[t+1]) / 4 from the voicing u = f0 > 0
        of the f0 this call decodes (before any shift; neighbours stay inside the utterance), so voiced frames keep alpha and a fully unvoiced
        frame alpha + (1 - alpha) * protect (tvc_convert_protect_f32 / tvc_convert_ragged_protect_f32).  alpha's forms (a float, B floats, an
        fp32 [B] / [1] device tensor), with or without alpha (None: 0), every target form, equal and ragged, auto_pitch and track; 0 is the
        alpha call bit for bit, None (the default) the call without it.  The 3-tap weight is an untuned guess: nobody has listened.
        `loudness` (extension; RVC's rms_mix_rate, as 1 - its value): make the converted wave follow that share of the loudness envelope of
        its source.  Every 10 ms the wave is scaled by (Es / Eo)^(share / 2), Es and Eo the mean powers of the padded input and of the wave
        over 50 ms: one more launch behind the conversion (tvc_loudness_match_f32), with no host synchronisation and capturable, equal and
        ragged batches alike (a ragged row's envelope never crosses its own padded length; the lengths travel as kernel arguments).  It runs
        in place on the wave when the batch has a row for every compute unit, and into a tensor of its own below that
        (engine.loudness_in_place).  A share in alpha's forms (a float in [0, 1], B of them, or an fp32 [B] / [1] device tensor, which the
        kernel clamps), or a feature_retrieval.LoudnessMatch with the settings (sub_frame must divide 480).  Every target form, with alpha,
        protect, auto_pitch, track and return_shift; 0 is the call without it bit for bit, None (the default) launch for launch.  The
        settings' defaults are guesses: nobody has listened.
        `limit` (extension): a look-ahead peak limiter behind everything else, loudness included: no sample of a row's own (padded) length
        leaves above the ceiling, exactly.  One more launch (tvc_limit_f32) into a tensor of its own, with no host synchronisation and
        capturable, equal and ragged batches alike.  A ceiling in dBFS (a number, or B of them; inf: off), an fp32 [B] / [1] device tensor
        of LINEAR ceilings, or a feature_retrieval.Limiter with the settings (sub_frame must divide 480).  Every target form, with every
        other keyword; None (the default) is the call without it, launch for launch.  The settings' defaults are guesses: nobody has listened.
        `carry` (extension, with a pitch path): a feature_retrieval.PitchCarry of B streams - row b's path starts from the scores the stream's
        last window left for this window's first frame, and leaves those of frame carry.hop_frames for the next (tvc_convert_carry_f32: the
        state is read and written in place, on the device, inside the same launch).  Equal batches only; ValueError without a pitch path, with
        `lengths=`, and for a carry of another size.  None (the default) is the call without it, launch for launch.
        `tune` (extension): pitch correction - the f0 the decoder's oscillator reads, behind the path, the register, the tracker and every
        shift, is snapped to a table of allowed notes: the note is chosen with hysteresis, the correction is smoothed by a retune time and a
        strength says how much of it is applied (one more launch directly in front of the decoder, in place, no workspace:
        tvc_tuned_convert_f32 / tvc_tuned_convert_ragged_f32; the definition is in include/tinyvc_hip.h and is exact: fp32, bit for bit what
        tests/helpers_pitch_snap.py computes).  A feature_retrieval.PitchSnap, or a string such as "A minor" / "chromatic" (PitchSnap's
        defaults).  Every target form, equal and ragged batches, with every other keyword; protect's voicing and the tracker keep reading the
        unshifted f0.  A strength of 0 is the call without it bit for bit, None (the default) launch for launch.  `tune_carry` (equal batches
        only): a feature_retrieval.SnapCarry of B streams - the note and the smoothed ratio travel from one window to the next, in place.
        The defaults are guesses: nobody has listened.
        `k` / `match_width` (extension; k is the reference's match_features(..., k), which its convert never passes): every frame becomes the
        mean over its k nearest index rows (1 .. 4: the fused search keeps four), neighbour e weighted by clamp(1 - (s_0 - s_e) /
        match_width, 0, 1) with s the cosine similarities the search already holds - one more instantiation of the merge + gather kernel,
        no new launch, no workspace (tvc_weighted_convert_f32 / tvc_weighted_convert_ragged_f32; the definition is in
        include/tinyvc_hip.h and is exact: bit for bit what tests/helpers_match_weight.py computes from the call's own similarities).  k: an
        int, B of them, or an int32 [B] / [1] device tensor; match_width: a float >= 0 in cosine units (inf: equal weights, 0: the nearest
        row alone), B of them, or an fp32 [B] / [1] device tensor.  [B] tensors are used in place and read when the kernel runs, which
        clamps k and treats a NaN or negative width as inf; host values outside the ranges are refused before any engine work.  Every
        target form (a Blend: every term's match), equal and ragged batches, with every other keyword.  k = 4 with match_width = inf is
        the call without them bit for bit, None for both (the default) launch for launch.  No width is suggested: nobody has listened.
        `continuity` (extension; unit selection's join cost): match along a path - the neighbour a frame's weights form around is chosen
        over the utterance as a whole (each row, each utterance of a ragged batch, each term of a Blend on its own), a neighbour gaining
        by its cosine to the query and by `continuity` times its cosine to the neighbour chosen for the frame before, so the anchor of a
        sharp match (k = 1 aside: that has no choice) stops alternating between two almost equally near rows.  A float >= 0, B of them,
        or an fp32 [B] / [1] device tensor used in place (the kernel reads NaN and negatives as 0); a host value > 0 without a finite
        host match_width or a width tensor is refused - under an infinite width it could have no effect.  Three launches in the gather's
        place (tvc_joined_convert_f32 / tvc_joined_convert_ragged_f32; the definition is in include/tinyvc_hip.h and is exact: bit for
        bit what tests/helpers_match_join.py computes).  0 is the call without it bit for bit, None (the default) launch for launch.
        No value is suggested: nobody has listened."""
        # 1. classify the target once; malformed targets, registers and shift lists are refused before any engine or device work
        B = wf.shape[0] if wf.dim() == 2 else 1
        auto = auto_pitch is not None and auto_pitch is not False
        if return_shift and not auto:
            raise ValueError("return_shift needs auto_pitch: without it the shifts are the caller's own pitch_shift")
        form = target_form(tgt)[0]
        if form == "blend":
            check_blend(tgt.terms, tgt._given, B)
        elif form == "table":
            check_references(tgt, B)
        regs = resolve_auto_pitch(auto_pitch, tgt, B) if auto else None
        if track is not None:
            if not auto:
                raise ValueError("track needs auto_pitch: the tracker finds the register the automatic shift starts from")
            if lengths is not None:
                raise ValueError("track with lengths: streams advance in lock step, there is no ragged form")
            if track.n_streams != B:
                raise ValueError(f"track: a tracker of {track.n_streams} streams for a batch of {B}")
            track.columns(-(-wf.shape[-1] // 480))      # the tracked columns must lie within the (padded) call's frames
        shift, shifts = pitch_shifts(pitch_shift, B)
        share = resolve_alpha(alpha, B) if alpha is not None else None
        guard = resolve_protect(protect, B) if protect is not None else None
        path = resolve_f0_estimation(f0_estimation)      # 'viterbi' or a PitchPath; every other name is None: the call it has always been
        if carry is not None:
            if path is None:
                raise ValueError("carry needs f0_estimation='viterbi' or a PitchPath: the state it carries is the pitch path's")
            if lengths is not None:
                raise ValueError("carry with lengths: streams advance in lock step, there is no ragged form")
            if carry.n_streams != B:
                raise ValueError(f"carry: a carry of {carry.n_streams} streams for a batch of {B}")
            if -(-wf.shape[-1] // 480) <= carry.hop_frames:
                raise ValueError(f"carry: hop_frames = {carry.hop_frames} must be below the call's {-(-wf.shape[-1] // 480)} frames")
        near = resolve_match_k(k, B) if k is not None else None
        wide = resolve_match_width(match_width, B) if match_width is not None else None
        along = resolve_continuity(continuity, B, wide) if continuity is not None else None
        weighted = near is not None or wide is not None or along is not None
        tune = resolve_tune(tune)
        if tune_carry is not None and lengths is not None:
            raise ValueError("tune_carry with lengths: streams advance in lock step, there is no ragged form")
        check_tune_carry(tune_carry, tune, B, -(-wf.shape[-1] // 480))
        level = resolve_loudness(loudness, B) if loudness is not None else None
        if level is not None and 480 % level[0].sub_frame:
            raise ValueError(f"loudness: sub_frame = {level[0].sub_frame} does not divide the 480-sample frames a call is padded to")
        bound = resolve_limit(limit, B) if limit is not None else None
        if bound is not None and 480 % bound[0].sub_frame:
            raise ValueError(f"limit: sub_frame = {bound[0].sub_frame} does not divide the 480-sample frames a call is padded to")
        # 2. the inputs, on the device
        wf = utils.autopad_waveform(self._input_device(wf))
        eng = self.engine(wf.device)
        B, L = wf.shape
        if noise_angle is not None:
            noise_angle = self._input_device(noise_angle)
        lens = _padded_lengths(lengths, B, L) if lengths is not None else None
        # 3. the target as prepared blobs: (blob, n) of a shared index, or the tables of B rows (x M terms and their weights for a blend)
        w = None
        if form == "blend":
            blobs, ns, w = tgt.resolve(B, wf.device, self._input_device)
        elif form == "table":
            blobs, ns = prepare_references([self._input_device(t) for t in tgt] if isinstance(tgt, (list, tuple)) else self._input_device(tgt))
        else:
            blobs, ns = prepare_reference(self._input_device(tgt))
            if auto or shifts is not None or share is not None or guard is not None or path is not None or tune is not None or weighted:      # a value per row (given, or found on the device): the shared blob in every row (one segment)
                form, blobs, ns = "table", [blobs] * B, [ns] * B
        # 4. one engine call
        pitch = shift if shifts is None else shifts
        if share is not None or guard is not None or path is not None or tune is not None or weighted:      # the alpha / protect / path / tuned / weighted entry covers every case below: plain shifts, target registers, a tracker
            rows = {"alpha": alpha_rows(share, B, wf.device) if share is not None else None}
            if guard is not None:
                rows["protect"] = protect_rows(guard, B, wf.device)
            if path is not None:
                rows["path"] = path
            if carry is not None:
                rows["carry"] = carry
            if tune is not None:
                rows["tune"], rows["tune_carry"] = tune, tune_carry
            if weighted:
                rows["neighbours"] = match_k_rows(near, B, wf.device) if near is not None else None
                rows["width"] = match_width_rows(wide, B, wf.device) if wide is not None else None
            if along is not None:
                rows["join"] = continuity_rows(along, B, wf.device)
            res = eng._convert("joined" if along is not None else "weighted" if weighted else "tuned" if tune is not None else "path" if path is not None else "alpha" if guard is None else "protect", wf, blobs, ns, pitch, noise_angle, lens, w,
                               target_registers(regs, B, wf.device) if auto else None, track=track, **rows)
            res = res if return_shift or not auto else res[0]
        elif not auto:
            res = eng._convert(form, wf, blobs, ns, pitch, noise_angle, lens, w)
        else:
            wave, sh = eng._convert("auto" if track is None else "track", wf, blobs, ns, pitch, noise_angle, lens, w, target_registers(regs, B, wf.device),
                                    track=track)
            res = (wave, sh) if return_shift else wave
        # 5. with loudness, one launch behind it: the padded input and the wave (in place where that is the faster form)
        if level is not None:
            wave = res[0] if isinstance(res, tuple) else res
            wave = eng.loudness_match(wf, wave, loudness_rows(level[1], B, wf.device), lengths=lens, settings=level[0],
                                      out=wave if loudness_in_place(B, wf.device) else None)
            res = (wave,) + tuple(res[1:]) if isinstance(res, tuple) else wave
        # 6. with limit, one launch behind that, into a tensor of its own (a tile reads its neighbours' samples: never in place)
        if bound is not None:
            wave = res[0] if isinstance(res, tuple) else res
            wave = eng.limit(wave, limit_rows(bound[1], B, wf.device), lengths=lens, settings=bound[0])
            res = (wave,) + tuple(res[1:]) if isinstance(res, tuple) else wave
        return res
