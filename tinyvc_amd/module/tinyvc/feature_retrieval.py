"""kNN-VC feature matching (reference module/tinyvc/feature_retrieval.py:15-33) on the streamed
top-k kernel of csrc/knn.hip."""
import collections
import ctypes
import math
import os
import sys

import torch

from ... import spec, stream_state
from ..._lib import PitchPathSettings, PitchSnapSettings
from ...engine import default_engine, integer, limiter_drive, limiter_geometry, loudness_geometry, loudness_levels


def prepare_reference(reference):
    """Normalise + repack an index [1, 768, N] once.  The prepared blob rides on the tensor object
    itself (keyed by its in-place version counter), so it lives exactly as long as the index and can
    never be confused with another tensor that later reuses the same device address."""
    hit = getattr(reference, "_tvc_prepared", None)
    if hit is not None and hit[0] == reference._version and hit[1] == str(reference.device):
        return hit[2], hit[3]
    eng = default_engine(reference.device)
    blob, n = eng.knn_prepare(reference)
    try:
        reference._tvc_prepared = (reference._version, str(reference.device), blob, n)
    except Exception:
        pass
    return blob, n


def index_columns(frames, stride, size, perm=None):
    """The reference's index recipe (extract_index.py:43-58) as a column plan, on the host: clips of frames[b] frames lie back to back in
    packed features [768, sum(frames)]; every `stride`-th frame of each clip in order, concatenated, index_select(perm), the first `size`
    -> the int64 columns of the packed features that make up the index, in its order.  perm (optional): a permutation - any index list -
    of the strided frames; size None = all of them.  Raises ValueError if a column would fall outside the packed features, before
    anything touches the device."""
    frames = [int(t) for t in frames]
    stride = int(stride)
    if stride < 1 or any(t < 1 for t in frames):
        raise ValueError("index_columns: stride >= 1 and at least one frame per clip")
    parts, off = [], 0
    for t in frames:
        parts.append(torch.arange(off, off + t, stride, dtype=torch.int64))
        off += t
    cols = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64)
    if perm is not None:
        perm = torch.as_tensor(perm).to("cpu", torch.int64).reshape(-1)
        if perm.numel() and (int(perm.min()) < 0 or int(perm.max()) >= cols.numel()):
            raise ValueError(f"index_columns: perm selects outside the {cols.numel()} strided frames")
        cols = cols.index_select(0, perm)
    if size is not None:
        if int(size) < 0:
            raise ValueError("index_columns: size must not be negative")
        cols = cols[:int(size)]
    if cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= off):
        raise ValueError(f"index_columns: a column outside the {off} packed frames")
    return cols.contiguous()


@torch.no_grad()
def build_index(generator, wf, lengths, stride=4, size=None, perm=None, half=False):
    """A speaker index from a batch of target clips in one pass on the device (the reference's extract_index.py:43-58 for clips already
    in memory): wf [B, L] with clip b in its first lengths[b] samples -> index [1, 768, N] (fp32, or fp16 with half=True), the tensor
    `assemble` of extract_index.py builds from one `encode` per clip.  Ragged encode, column plan (index_columns), one gather that writes
    the index AND its prepared blob: the blob rides on the returned tensor like prepare_reference's, so the first convert /
    match_features against it prepares nothing."""
    ssl, f0, pre = generator.encode_packed(wf, lengths)
    cols = index_columns([pre[b + 1] - pre[b] for b in range(len(pre) - 1)], stride, size, perm)
    index = index_from_columns(generator.engine(ssl.device), ssl, cols, half)
    # the speaker's pitch register over ALL frames of the clips (not the strided selection): what convert(auto_pitch=True) aims at
    index.pitch_register = pitch_register(f0, [f0.numel()])
    return index


def index_from_columns(eng, feats, cols, half=False):
    """feats [768, S] on the device, cols (host or device int64) -> index [1, 768, N] carrying its prepared blob (Engine.knn_prepare_columns)."""
    blob, n, index = eng.knn_prepare_columns(feats, cols, half=half, want_index=True)
    index._tvc_prepared = (index._version, str(index.device), blob, n)
    return index


@torch.no_grad()
def compact_index(reference, size, iters=8, generator=None, init_cols=None, snap=False, return_info=False):
    """A smaller index by k-means instead of truncation: reference [1, 768, N] (fp32 or fp16) -> [1, 768, size] fp32, the centroids of
    `iters` rounds of (cosine assignment, raw-mean update) on the device (Engine.index_compact), started from the vectors init_cols
    (default: torch.randperm(N, generator=generator)[:size]).  The reference's recipe (extract_index.py:43-58) reaches a size by dropping
    vectors; this keeps the mean of every group of similar ones.  The prepared blob rides on the result like index_from_columns'.
    snap=True replaces each centroid by its nearest vector of `reference` (cosine): the result then holds real frames of the speaker, not
    averages.  return_info=True -> (index, {"assign", "counts", "moved"}): the last assignment [N], the cluster sizes [size] and the points
    that changed cluster in each round [iters]."""
    if not isinstance(reference, torch.Tensor) or reference.dim() != 3 or reference.shape[0] != 1 or reference.shape[1] != 768:
        raise ValueError(f"compact_index: reference must be [1, 768, N], got {tuple(getattr(reference, 'shape', ()))}")
    N, size = reference.shape[2], int(size)
    if not 4 <= size <= N:
        raise ValueError(f"compact_index: need 4 <= size <= N, got size = {size}, N = {N}")
    if init_cols is None:
        init_cols = torch.randperm(N, generator=generator)[:size]
    init_cols = torch.as_tensor(init_cols).to(torch.int64).reshape(-1)
    if init_cols.numel() != size or int(init_cols.min()) < 0 or int(init_cols.max()) >= N:
        raise ValueError(f"compact_index: init_cols must be {size} point numbers in [0, {N})")
    eng = default_engine(reference.device)
    blob, n = prepare_reference(reference)
    index, cblob, assign, counts, moved = eng.index_compact(blob, n, init_cols, iters)
    if snap:
        _sims, idx = eng.knn_topk(index, blob, n)
        cblob, _k, index = eng.knn_prepare_columns(reference[0].float(), idx[0, :, 0], half=False, want_index=True)
    index._tvc_prepared = (index._version, str(index.device), cblob, size)
    return (index, {"assign": assign, "counts": counts, "moved": moved}) if return_info else index


# ---- pitch registers: the other half of a target (convert(auto_pitch=...)) -------------------------------------------------------------
PitchRegister = collections.namedtuple("PitchRegister", ["median_hz", "voiced"])      # device tensors [rows]: fp32 Hz, int32 voiced frames


@torch.no_grad()
def pitch_register(f0, lengths=None):
    """The pitch register of rows of f0 on the device (Engine.pitch_match): the lower median of each row's voiced frames,
    torch.median(row[row > 0]) bit for bit, and their count -> PitchRegister(median_hz [rows] fp32 - 0 for a row without a voiced frame -,
    voiced [rows] int32).  f0 [B, 1, T] / [B, T]: one register per row.  lengths (frames): f0 is packed (encode_packed's [S]), row b
    owns the lengths[b] values behind those of the rows before it; lengths = [S] is the register of everything."""
    eng = default_engine(f0.device)
    row_start = None
    if lengths is not None:
        row_start = [0]
        for n in lengths:
            row_start.append(row_start[-1] + int(n))
    med, voiced, _sh, _ = eng.pitch_match(f0, row_start)
    return PitchRegister(med, voiced)


def semitones_between(src_hz, tgt_hz):
    """12 * log2(tgt_hz / src_hz) in fp64 on the host: the automatic shift of tvc_pitch_match_f32 without its offset.  Floats -> a float;
    sequences / tensors -> a list.  A pair with src_hz <= 0 or tgt_hz <= 0 (no register) or NaN gives 0.0, as on the device."""
    def one(a, b):
        a, b = float(a), float(b)
        return 12.0 * math.log2(b / a) if a > 0.0 and b > 0.0 else 0.0

    def seq(x):
        if isinstance(x, torch.Tensor):
            return x.detach().to("cpu", torch.float64).reshape(-1).tolist()
        return list(x) if hasattr(x, "__len__") else None

    a, b = seq(src_hz), seq(tgt_hz)
    if a is None and b is None:
        return one(src_hz, tgt_hz)
    n = len(a) if a is not None else len(b)
    a = a if a is not None else [src_hz] * n
    b = b if b is not None else [tgt_hz] * n
    if len(a) != len(b):
        raise ValueError(f"semitones_between: {len(a)} source registers against {len(b)} targets")
    return [one(x, y) for x, y in zip(a, b)]


def sidecar_path(index_path):
    """where the register of the index file `index_path` lives: <index_path>.f0.pt"""
    return str(index_path) + ".f0.pt"


def save_register(index_path, register):
    """writes {"median_hz": float, "voiced": int} beside the index file (the index file itself keeps the reference's format)"""
    torch.save({"median_hz": float(register.median_hz.reshape(-1)[0]), "voiced": int(register.voiced.reshape(-1)[0])}, sidecar_path(index_path))


def attach_register(index, index_path):
    """index.pitch_register <- the sidecar of `index_path` when there is one (tensors on the index's device); returns index"""
    path = sidecar_path(index_path)
    if os.path.exists(path):
        d = torch.load(path, map_location="cpu")
        index.pitch_register = PitchRegister(torch.tensor([float(d["median_hz"])], dtype=torch.float32, device=index.device),
                                             torch.tensor([int(d["voiced"])], dtype=torch.int32, device=index.device))
    return index


def _registers_of(tgt):
    """the [rows] median tensors that ride on a target (a tensor or a list of tensors), or ValueError naming the one without"""
    items = list(tgt) if isinstance(tgt, (list, tuple)) else [tgt]
    out = []
    for i, t in enumerate(items):
        reg = getattr(t, "pitch_register", None)
        if reg is None:
            raise ValueError(f"auto_pitch=True: target{f' {i}' if len(items) > 1 else ''} carries no pitch register (build_index and the entry scripts' "
                             "loaders attach one; else pass auto_pitch in Hz)")
        out.append(reg.median_hz.reshape(-1))
    return out


def resolve_auto_pitch(auto_pitch, tgt, B):
    """convert's auto_pitch -> what becomes the [B] device tensor of target registers, checked on the host (no engine, no device work):
    a float in Hz, a [B] or [1] tensor, or True = the registers riding on the target tensor(s).  Returns a float or a list of tensors
    whose concatenation has 1 or B entries; raises ValueError otherwise."""
    if auto_pitch is True:
        if isinstance(tgt, Blend):
            raise ValueError("auto_pitch=True with a Blend: its weights live on the device, so the blend's register is the caller's to give (auto_pitch in Hz)")
        regs = _registers_of(tgt)
        n = sum(r.numel() for r in regs)
        if n not in (1, B):
            raise ValueError(f"auto_pitch=True: {n} target registers for a batch of {B}")
        return regs
    if isinstance(auto_pitch, torch.Tensor):
        if auto_pitch.dim() > 1 or auto_pitch.numel() not in (1, B):
            raise ValueError(f"auto_pitch: a tensor of 1 or B = {B} registers in Hz, got {tuple(auto_pitch.shape)}")
        return [auto_pitch.reshape(-1)]
    if isinstance(auto_pitch, bool) or not isinstance(auto_pitch, (int, float)):
        raise ValueError(f"auto_pitch: a register in Hz (float or [B] / [1] tensor) or True, got {auto_pitch!r}")
    return float(auto_pitch)


def target_registers(resolved, B, device):
    """resolve_auto_pitch's result as the contiguous fp32 [B] device tensor the engine takes (a [B] fp32 device tensor passes through as it
    is: the kernels read it when they run)"""
    if isinstance(resolved, float):
        return torch.full((B,), resolved, dtype=torch.float32, device=device)
    t = resolved[0] if len(resolved) == 1 else torch.cat([r.to(device) for r in resolved])
    t = t.to(device=device, dtype=torch.float32)
    return (t.expand(B) if t.numel() == 1 else t).contiguous()


def resolve_alpha(alpha, B, name="alpha"):
    """convert's alpha - the share of a row's own content features that survives the match (the reference's match_features(..., alpha);
    RVC's index rate is 1 - alpha) - checked on the host (no engine, no device work): a float, a sequence of B (or 1) floats, or a 1-D fp32
    tensor of B or 1 entries ON THE DEVICE (the kernels read it when they run).  Returns a list of B floats, or the tensor; raises
    ValueError naming alpha otherwise.  Values are neither clamped nor normalised: below 0 and above 1 extrapolate.
    `name`: the other per-row value of this form, "protect" (resolve_protect), under its own name in every message."""
    if isinstance(alpha, torch.Tensor):
        if alpha.dim() != 1 or alpha.numel() not in (1, B):
            raise ValueError(f"{name}: a tensor of 1 or B = {B} shares, got shape {tuple(alpha.shape)}")
        if alpha.dtype != torch.float32:
            raise ValueError(f"{name}: an fp32 tensor (it is read in place by the kernels, never converted), got {alpha.dtype}")
        if alpha.device.type != "cuda":
            raise ValueError(f"{name}: a tensor lives on the GPU, where the kernels read it when they run; got one on {alpha.device} (pass floats instead)")
        return alpha
    if isinstance(alpha, (list, tuple)):
        vals = list(alpha)
        if len(vals) not in (1, B):
            raise ValueError(f"{name}: {len(vals)} shares for a batch of {B}")
    else:
        vals = [alpha]
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, (int, float)):
            raise ValueError(f"{name}: a float, a sequence of one float per row or an fp32 [B] / [1] device tensor, got {alpha!r}")
    return [float(x) for x in vals] * (B if len(vals) == 1 else 1)


def alpha_rows(resolved, B, device, name="alpha"):
    """resolve_alpha's result as the contiguous fp32 [B] device tensor the engine takes (a [B] tensor on `device` passes through as it is,
    so in-place changes reach a captured graph; a [1] tensor is expanded to a new [B] one)"""
    if isinstance(resolved, torch.Tensor):
        device = torch.device(device)
        if resolved.device.type != device.type or (device.index is not None and resolved.device.index != device.index):
            raise ValueError(f"{name}: the tensor is on {resolved.device}, the conversion runs on {device}")
        return (resolved.expand(B) if resolved.numel() != B else resolved).contiguous()
    return torch.tensor(resolved, dtype=torch.float32, device=device)


def resolve_protect(protect, B):
    """convert's protect - how far the source's share rises on UNVOICED frames: frame t keeps a_t = a + (1 - a) * (protect * w[t]) of the row's
    own content features, w[t] in {0, .25, .5, .75, 1} the unvoiced weight of the frame and its two neighbours in the f0 the call decodes
    (include/tinyvc_hip.h; 1 - RVC's protect value) - in alpha's forms, by alpha's code, refused under its own name"""
    return resolve_alpha(protect, B, "protect")


def protect_rows(resolved, B, device):
    return alpha_rows(resolved, B, device, "protect")


def resolve_match_k(k, B):
    """convert's k - how many of the four nearest index rows a frame averages (the reference's match_features(..., k); the fused match keeps
    four, so 1 .. 4) - checked on the host: an int in 1 .. 4, a sequence of B (or 1) of them, or a 1-D int32 tensor of B or 1 entries ON THE
    DEVICE, taken as it is (the kernel clamps it to 1 .. 4 when it runs).  Returns a list of B ints, or the tensor; ValueError naming k
    otherwise."""
    if isinstance(k, torch.Tensor):
        if k.dim() != 1 or k.numel() not in (1, B):
            raise ValueError(f"k: a tensor of 1 or B = {B} entries, got shape {tuple(k.shape)}")
        if k.dtype != torch.int32:
            raise ValueError(f"k: an int32 tensor (it is read in place by the kernels, never converted), got {k.dtype}")
        if k.device.type != "cuda":
            raise ValueError(f"k: a tensor lives on the GPU, where the kernels read it when they run; got one on {k.device} (pass ints instead)")
        return k
    vals = list(k) if isinstance(k, (list, tuple)) else [k]
    if len(vals) not in (1, B):
        raise ValueError(f"k: {len(vals)} values for a batch of {B}")
    for x in vals:
        if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= 4:
            raise ValueError(f"k: an int in 1 .. 4 (the fused match keeps four neighbours; match_features serves any k), one per row or an int32 [B] / [1] device "
                             f"tensor, got {k!r}")
    return [int(x) for x in vals] * (B if len(vals) == 1 else 1)


def match_k_rows(resolved, B, device):
    """resolve_match_k's result as the contiguous int32 [B] device tensor the engine takes (a [B] tensor passes through as it is)"""
    if isinstance(resolved, torch.Tensor):
        return alpha_rows(resolved, B, device, "k")
    return torch.tensor(resolved, dtype=torch.int32, device=device)


def resolve_match_width(width, B):
    """convert's match_width - the similarity width of the weighted match, in cosine units: neighbour e of a frame weighs
    clamp(1 - (s_0 - s_e) / width, 0, 1), s the cosine similarities (include/tinyvc_hip.h) - in alpha's forms: a float >= 0 (inf: equal
    weights; 0: the nearest row and its exact ties), B of them, or an fp32 [B] / [1] device tensor, taken as it is.  A negative or NaN host
    value is refused under its own name."""
    res = resolve_alpha(width, B, "match_width")
    if not isinstance(res, torch.Tensor):
        for x in res:
            if not x >= 0.0:
                raise ValueError(f"match_width: a width in cosine units is >= 0 (inf: equal weights), got {x!r}")
    return res


def match_width_rows(resolved, B, device):
    return alpha_rows(resolved, B, device, "match_width")


def resolve_continuity(continuity, B, width=None):
    """convert's continuity - the weight c of the match along a path: the neighbour a frame's weights form around is chosen over the
    utterance as a whole, a neighbour gaining by its cosine to the query and by c times its cosine to the neighbour chosen for the frame
    before (include/tinyvc_hip.h) - in alpha's forms: a float >= 0 (0: every frame on its own), B of them, or an fp32 [B] / [1] device
    tensor, taken as it is (the kernel reads a NaN or negative value as 0).  A negative or NaN host value is refused under its own name.
    `width`: resolve_match_width's result for the same call, or None - a host continuity > 0 with no finite host match_width and no
    width tensor is refused too: under an infinite width every neighbour weighs 1 wherever the path goes, so it could have no effect.
    The check is per call, not per row: one finite width anywhere passes every row's continuity, and k = 1, which has no choice to make
    either, is not looked at - the refusal catches the keyword given alone, not every setting without an effect."""
    res = resolve_alpha(continuity, B, "continuity")
    if isinstance(res, torch.Tensor):
        return res
    for x in res:
        if not x >= 0.0:
            raise ValueError(f"continuity: a weight on the cosine between neighbouring frames' rows is >= 0, got {x!r}")
    if any(x > 0.0 for x in res) and not isinstance(width, torch.Tensor) and not (width is not None and any(math.isfinite(w) for w in width)):
        raise ValueError("continuity > 0 needs a finite match_width (or a match_width tensor): under an infinite width every neighbour weighs "
                         "1 wherever the path goes, and continuity could have no effect")
    return res


def continuity_rows(resolved, B, device):
    return alpha_rows(resolved, B, device, "continuity")


class LoudnessMatch:
    """convert's loudness - how far the converted wave follows the loudness envelope of its source (tvc_loudness_match_f32; the definition is
    in include/tinyvc_hip.h; 1 - RVC's rms_mix_rate): every `sub_frame` samples the output is scaled by (Es / Eo)^(share / 2), Es and Eo the
    mean powers of input and output over 2 * smooth + 1 sub-frames, never below `floor_db` (dB re full scale: silence is not amplified),
    never by more than `boost_db` up or `cut_db` down, ramped from sub-frame to sub-frame.
      share      alpha's forms: a float, B floats, or an fp32 [B] / [1] device tensor ([B]: used in place, read when the kernel runs, where
                 values outside [0, 1] are clamped); 0 leaves every bit
      sub_frame  24 kHz samples, a multiple of 4 (convert: a divisor of 480); smooth: sub-frames each side, 0 .. 32
    The defaults are guesses: nobody has listened to them yet.  The settings are checked here and the share in resolve_loudness
    (ValueError), before any engine work."""

    def __init__(self, share, sub_frame=240, smooth=2, floor_db=-60.0, boost_db=12.0, cut_db=40.0):
        try:
            sub_frame = integer(sub_frame, "loudness geometry", "sub")
            loudness_geometry(sub_frame, sub_frame, smooth)      # one sub-frame: the limits of sub_frame and smooth themselves
        except ValueError as e:
            raise ValueError(f"loudness: {e}") from None
        self.floor_db, self.boost_db, self.cut_db = loudness_levels(floor_db, boost_db, cut_db)
        self.share, self.sub_frame, self.smooth = share, int(sub_frame), int(smooth)


def resolve_loudness(loudness, B):
    """convert's loudness as given - a LoudnessMatch, or a bare share (LoudnessMatch(share)) - checked on the host (no engine, no device work)
    -> (settings, share): the LoudnessMatch and its share as a list of B floats or the device tensor.  The share takes alpha's forms by
    alpha's code; floats outside [0, 1] and NaN are refused (a tensor is read, and clamped, on the device).  ValueError naming loudness."""
    settings = loudness if isinstance(loudness, LoudnessMatch) else LoudnessMatch(loudness)
    share = resolve_alpha(settings.share, B, "loudness")
    if not isinstance(share, torch.Tensor) and not all(0.0 <= x <= 1.0 for x in share):
        raise ValueError(f"loudness: a share of the source's envelope in [0, 1], got {settings.share!r}")
    return settings, share


def loudness_rows(resolved, B, device):
    return alpha_rows(resolved, B, device, "loudness")


def add_loudness_argument(parser):
    """`--loudness E` for the entry scripts' parsers: absent (None) is the call without it"""
    parser.add_argument("--loudness", type=float, default=None, metavar="E",
                        help="make the converted voice follow this share (0 .. 1) of the source's loudness envelope, 10 ms sub-frames smoothed over "
                             "50 ms (1 - RVC's rms_mix_rate).  The defaults behind it are guesses: nobody has listened.  default: absent, the level "
                             "the decoder gives")


def loudness_keywords(args, script):
    """what `--loudness` adds to the script's convert call: nothing when it is absent (the call is today's), else {"loudness": E} and one
    printed line; a value outside [0, 1] ends the script"""
    e = getattr(args, "loudness", None)
    if e is None:
        return {}
    if not 0.0 <= e <= 1.0:      # (NaN fails both)
        sys.exit(f"{script}: --loudness must be a share in 0 .. 1")
    print(f"Following {e:g} of the source's loudness envelope (loudness; rms mix rate {1 - e:g})")
    return {"loudness": float(e)}


def limit_ceiling(db, what="limit"):
    """a ceiling in dBFS as the linear amplitude the limiter's kernels read: 10^(db / 20), the one place it is computed - in double, on
    the host; the device never takes a power of ten of it.  +inf is off (inf).  ValueError for anything that is no number of dB in
    -600 .. 600 or +inf."""
    if isinstance(db, bool) or not isinstance(db, (int, float)) or not (db == math.inf or -600.0 <= db <= 600.0):
        raise ValueError(f"{what}: a ceiling is a number of dBFS in -600 .. 600, or inf for none; got {db!r}")
    return math.inf if db == math.inf else 10.0 ** (float(db) / 20.0)


class Limiter:
    """convert's limit - the look-ahead peak limiter behind everything else (tvc_limit_f32; the definition is in include/tinyvc_hip.h): no
    sample of the result lies above the ceiling, exactly.  The gain falls at once, one sub-frame ahead of a peak, and rises linearly.
      ceiling_db    dBFS: a number, B numbers (inf: off), or an fp32 [B] / [1] device tensor of LINEAR ceilings ([B]: used in place, read
                    when the kernel runs; NaN, <= 0 and inf are off)
      sub_frame     24 kHz samples, a multiple of 4 (convert: a divisor of 480): the look-ahead and the attack; 24 = 1 ms
      release_size  24 kHz samples, 1 .. 4096 whole sub-frames: the time a gain of 0 takes back to 1
      drive_db      a gain in front of the limiter
    The defaults are guesses: nobody has listened to them yet.  The settings are checked here and the ceiling in resolve_limit
    (ValueError), before any engine work."""

    def __init__(self, ceiling_db=-1.0, sub_frame=24, release_size=2400, drive_db=0.0):
        self.sub_frame, self.release, self.drive_db = limiter_settings(sub_frame, release_size, drive_db, "limit")
        self.ceiling_db, self.release_size = ceiling_db, int(release_size)


def limiter_settings(sub_frame, release_size, drive_db, what, block_size=None):
    """a limiter's host settings, checked by the library's own rule -> (sub_frame, release in sub-frames, drive_db as fp32); `block_size`:
    a stream's block.  ValueError naming `what`."""
    try:
        sub_frame, release_size = integer(sub_frame, "limiter geometry", "sub"), integer(release_size, "limiter geometry", "release_size")
        limiter_geometry(sub_frame, sub_frame, 1)      # the limits of sub_frame itself
        if release_size % sub_frame:
            raise ValueError(f"release_size = {release_size} is not a whole number of {sub_frame}-sample sub-frames")
        limiter_geometry(sub_frame if block_size is None else block_size, sub_frame, release_size // sub_frame, stream_block=block_size is not None)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    return sub_frame, release_size // sub_frame, limiter_drive(drive_db, what)


def resolve_limit(limit, B):
    """convert's limit as given - a Limiter, or a bare ceiling (Limiter(ceiling)) - checked on the host (no engine, no device work) ->
    (settings, ceiling): the Limiter and its ceiling as a list of B LINEAR floats or the device tensor (linear already).  The ceiling takes
    alpha's forms by alpha's code; the dB to linear conversion happens here, once.  ValueError naming limit."""
    settings = limit if isinstance(limit, Limiter) else Limiter(limit)
    ceiling = resolve_alpha(settings.ceiling_db, B, "limit")
    if not isinstance(ceiling, torch.Tensor):
        ceiling = [limit_ceiling(x) for x in ceiling]
    return settings, ceiling


def limit_rows(resolved, B, device):
    return alpha_rows(resolved, B, device, "limit")


def add_limit_argument(parser):
    """`--limit [DB]` for the entry scripts' parsers: absent (None) is the run without it, bare is -1 dBFS"""
    parser.add_argument("--limit", type=float, nargs="?", const=-1.0, default=None, metavar="DB",
                        help="hold every output sample at or below this ceiling (dBFS; bare: -1) with a look-ahead peak limiter on the device, "
                             "1 ms ahead of a peak, behind everything else.  The defaults behind it are guesses: nobody has listened.  default: "
                             "absent, the output is not bounded")


def limit_keywords(args, script):
    """what `--limit` adds to the script's convert call: nothing when it is absent (the call is today's), else {"limit": DB} and one
    printed line; a value that is no ceiling ends the script"""
    db = getattr(args, "limit", None)
    if db is None:
        return {}
    try:
        c = limit_ceiling(db, "--limit")
    except ValueError as e:
        sys.exit(f"{script}: {e}")
    print(f"Limiting peaks to {db:g} dBFS ({c:.6g} of full scale; 1 ms look-ahead)")
    return {"limit": float(db)}


def _f32(x):
    return ctypes.c_float(x).value


class PitchPath:
    """convert's f0_estimation='viterbi' - the pitch path, a Viterbi decode of the call's own pitch logits over each utterance as a whole in
    the place of the per-frame top-4 expectation (tvc_pitch_path_f32 and the *_path_f32 conversions; the definition is in
    include/tinyvc_hip.h).  Host values, baked into a captured graph:
      step      cost per class of distance inside the band (>= 0, finite)
      band      classes a voiced frame may move at `step` each, 0 .. 32 (48 classes are one octave, a frame is 20 ms)
      jump      cost of any longer move between voiced classes (>= band * step; inf allowed)
      voicing   cost of a move between unvoiced (class 0) and voiced (>= 0; inf allowed)
      refine    the frequency is a local expectation over the classes within `refine` of the path's, 0 .. 4 (0: the class frequency itself)
    The defaults are guesses: nobody has listened to them yet.  Checked here (ValueError), by the library's own rule on the fp32 values,
    before any engine work."""
    MAX_BAND, MAX_REFINE = 32, 4

    def __init__(self, step=0.5, band=12, jump=12.0, voicing=3.0, refine=2):
        for name, x in (("step", step), ("jump", jump), ("voicing", voicing)):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or math.isnan(x):
                raise ValueError(f"f0_estimation: {name} must be a number, got {x!r}")
        band, refine = integer(band, "f0_estimation", "band"), integer(refine, "f0_estimation", "refine")
        step, jump, voicing = _f32(step), _f32(jump), _f32(voicing)
        if not (0.0 <= step < math.inf):
            raise ValueError(f"f0_estimation: step must be finite and >= 0, got {step!r}")
        if not 0 <= band <= self.MAX_BAND:
            raise ValueError(f"f0_estimation: band must lie in 0 .. {self.MAX_BAND}, got {band}")
        if not jump >= _f32(band * step):
            raise ValueError(f"f0_estimation: jump must be >= band * step = {_f32(band * step):g} (inf is allowed), got {jump!r}")
        if not voicing >= 0.0:
            raise ValueError(f"f0_estimation: voicing must be >= 0 (inf is allowed), got {voicing!r}")
        if not 0 <= refine <= self.MAX_REFINE:
            raise ValueError(f"f0_estimation: refine must lie in 0 .. {self.MAX_REFINE}, got {refine}")
        self.step, self.band, self.jump, self.voicing, self.refine = step, band, jump, voicing, refine

    def params(self):
        """the five settings as a tuple: what a captured graph has baked in"""
        return (self.step, self.band, self.jump, self.voicing, self.refine)

    def settings(self):
        """the tvc_pitch_path struct the library takes"""
        return PitchPathSettings(*self.params())

    def __repr__(self):
        return "PitchPath(step={}, band={}, jump={}, voicing={}, refine={})".format(*self.params())


class PitchCarry:
    """The pitch path's state of a set of streams that advance in lock step (tvc_pitch_path_carry_f32 / tvc_convert_carry_f32; the
    definition is in include/tinyvc_hip.h): a stream's window advances by `hop_frames` = block_size / 480 frames per block, so frame
    hop_frames of one window is frame 0 of the next - the same instant.
      scores [S, 512] fp32   the best-predecessor values of that frame (maximum exactly 0; zeros: a fresh path), on the device
    Every block the path kernel adds a stream's scores to its window's first emissions and leaves the new ones in their place: the forward
    recursion of an online Viterbi, so a window no longer starts from a flat prior.  The scores are a prior whose spread the costs bound
    (no class lies further than about max(jump, voicing) behind the best), not the decode of any single logits tensor: every window has
    logits of its own.  Whatever is written into `scores`, the kernel takes values <= 0 only and counts the rest as 0.  Every argument is
    checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, hop_frames, device=None):
        for x, name in ((n_streams, "n_streams"), (hop_frames, "hop_frames")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1 or x > 0x7fffffff:
                raise ValueError(f"PitchCarry: {name} must be an integer >= 1, got {x!r}")
        self.n_streams, self.hop_frames = n_streams, hop_frames
        self.device = gpu_device(device, "PitchCarry: the state lives on the GPU (device='cpu' builds a carry no engine will take)", cpu_ok=True)
        stream_state.allocate(self, stream_state.CARRY_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in"""
        return (self.hop_frames,)

    def reset(self, streams=None):
        """Start the path of every stream, or of the listed ones, afresh: in-place ops on the state tensor, so it works between replays of a
        captured graph (which reads it when it runs)."""
        stream_state.reset(self, stream_state.CARRY_STATE, streams)


def check_f0_carry(f0_carry, f0_estimation, block_size, n_streams):
    """a stream's f0_carry against everything that can be said on the host (ValueError, before anything is allocated) -> None (no carry),
    True (build one in init_buffer) or the PitchCarry given"""
    if f0_carry is None or f0_carry is False:
        return None
    if f0_carry is not True and not isinstance(f0_carry, PitchCarry):
        raise ValueError(f"f0_carry: True, False or a feature_retrieval.PitchCarry, got {type(f0_carry).__name__}")
    if resolve_f0_estimation(f0_estimation) is None:
        raise ValueError("f0_carry needs f0_estimation='viterbi' or a PitchPath: the state it carries is the pitch path's")
    if block_size % 480:
        raise ValueError(f"f0_carry: block_size = {block_size} is not a whole number of 480-sample frames (the window must advance by whole frames)")
    if f0_carry is not True and (f0_carry.n_streams, f0_carry.hop_frames) != (n_streams, block_size // 480):
        raise ValueError(f"f0_carry: a carry of {f0_carry.n_streams} streams advancing {f0_carry.hop_frames} frames, the streams are {n_streams} "
                         f"advancing {block_size // 480}")
    return f0_carry


SNAP_NOTES = 128      # TVC_PITCH_SNAP_NOTES
SCALES = {"chromatic": tuple(range(12)), "major": (0, 2, 4, 5, 7, 9, 11), "minor": (0, 2, 3, 5, 7, 8, 10), "pentatonic": (0, 2, 4, 7, 9)}
KEYS = {"C": 0, "C#": 1, "Db": 1, "D": 2, "D#": 3, "Eb": 3, "E": 4, "F": 5, "F#": 6, "Gb": 6, "G": 7, "G#": 8, "Ab": 8, "A": 9, "A#": 10, "Bb": 10, "B": 11}


def note_table(key="C", scale="major", notes=None, a4=440.0, low=24, high=96):
    """The table of allowed notes, on the host: MIDI low .. high filtered by the scale (or `notes`, an explicit list of MIDI numbers), each
    a4 * 2^((m - 69) / 12) in fp64 rounded to fp32 -> (a list of SNAP_NOTES floats, ascending, padded with inf; the number of notes).
    ValueError for anything it cannot build."""
    if isinstance(a4, bool) or not isinstance(a4, (int, float)) or not (0.0 < a4 < math.inf):
        raise ValueError(f"tune: a4 must be a positive finite number of Hz, got {a4!r}")
    if notes is not None:
        midi = list(notes) if isinstance(notes, (list, tuple, range)) else None
        if not midi or any(isinstance(m, bool) or not isinstance(m, int) or not 0 <= m <= 127 for m in midi):
            raise ValueError(f"tune: notes must be a non-empty list of MIDI numbers 0 .. 127, got {notes!r}")
        midi = sorted(set(midi))
    else:
        if key not in KEYS:
            raise ValueError(f"tune: key must be one of {', '.join(KEYS)}, got {key!r}")
        if scale not in SCALES:
            raise ValueError(f"tune: scale must be one of {', '.join(SCALES)}, got {scale!r}")
        for x, name in ((low, "low"), (high, "high")):
            if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= 127:
                raise ValueError(f"tune: {name} must be a MIDI number 0 .. 127, got {x!r}")
        degrees = {(KEYS[key] + d) % 12 for d in SCALES[scale]}
        midi = [m for m in range(low, high + 1) if m % 12 in degrees]
        if not midi:
            raise ValueError(f"tune: no note of {key} {scale} lies in MIDI {low} .. {high}")
    if len(midi) > SNAP_NOTES:
        raise ValueError(f"tune: {len(midi)} notes; the table holds {SNAP_NOTES}")
    hz = [_f32(float(a4) * 2.0 ** ((m - 69) / 12.0)) for m in midi]
    if not (hz[0] > 0.0 and hz[-1] < math.inf and all(a < b for a, b in zip(hz, hz[1:]))):
        raise ValueError(f"tune: a4 = {a4!r} gives notes that are not positive, finite and ascending in fp32")
    return hz + [math.inf] * (SNAP_NOTES - len(hz)), len(hz)


def parse_tune(text):
    """'A minor', 'chromatic', 'F#' -> (key, scale): a key (default C) and a scale (default major), in that order"""
    words = text.split() if isinstance(text, str) else []
    if len(words) == 1 and words[0] in SCALES:
        return "C", words[0]
    if len(words) == 1 and words[0] in KEYS:
        return words[0], "major"
    if len(words) == 2 and words[0] in KEYS and words[1] in SCALES:
        return words[0], words[1]
    raise ValueError(f"tune: 'KEY SCALE' with KEY one of {', '.join(KEYS)} and SCALE one of {', '.join(SCALES)} (either alone will do), got {text!r}")


class PitchSnap:
    """Pitch correction (convert's and the streams' `tune`; tvc_pitch_snap_f32 and the tvc_tuned_convert* entries; the definition is in
    include/tinyvc_hip.h): the f0 the decoder reads is snapped to a table of allowed notes.
      key, scale         the table is MIDI low .. high filtered by the scale (chromatic, major, minor, pentatonic) in that key;
      notes              ... or an explicit list of MIDI numbers;  a4: the pitch of MIDI 69 in Hz.  At most 128 notes.
      retune_ms          the time constant of the correction's one-pole smoother: g = 1 - exp(-20 / retune_ms) per 20 ms frame, 0 ms is g = 1
                         (vibrato passes while the note's centre moves; 0 flattens it)
      strength           how much of the correction is applied, 0 .. 1: a number, or one per row
      hysteresis_cents   a pitch leaves its note only that far beyond the bound to the next, 0 .. 100 (h = 2^(cents / 1200))
    f_min is the lowest note a semitone down (not below 32 Hz), f_max the highest a semitone up: frames outside pass untouched.
    `notes` and `strength` are tensors the kernel reads when it runs (on the device once the snap is bound to its rows: convert and
    init_buffer do that): `snap.notes.copy_(...)`, `snap.strength.fill_(...)` and `set_scale(...)` take effect in place, under a captured
    graph too.  The kernel finds the table's size itself, so whatever is written there gives pitches, never a fault.  h, g, f_min and
    f_max are host values, baked into a capture.  Every argument is checked here (ValueError) before any engine work.
    THE DEFAULTS ARE GUESSES: nobody has listened."""

    def __init__(self, key="C", scale="major", notes=None, a4=440.0, low=24, high=96, retune_ms=60.0, strength=1.0, hysteresis_cents=25.0, device=None):
        table, n = note_table(key, scale, notes, a4, low, high)
        for x, name in ((retune_ms, "retune_ms"), (hysteresis_cents, "hysteresis_cents")):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not (0.0 <= x < math.inf):
                raise ValueError(f"tune: {name} must be a finite number >= 0, got {x!r}")
        if hysteresis_cents > 100.0:
            raise ValueError(f"tune: hysteresis_cents must lie in 0 .. 100 (a semitone), got {hysteresis_cents!r}")
        rows = list(strength) if isinstance(strength, (list, tuple)) else [strength]
        if not rows or any(isinstance(s, bool) or not isinstance(s, (int, float)) or not 0.0 <= s <= 1.0 for s in rows):
            raise ValueError(f"tune: strength must be a number in 0 .. 1, or a list of them (one per row), got {strength!r}")
        self.retune = _f32(1.0 if retune_ms == 0 else 1.0 - math.exp(-20.0 / retune_ms))
        self.hysteresis = _f32(2.0 ** (hysteresis_cents / 1200.0))
        if not 0.0 < self.retune <= 1.0:
            raise ValueError(f"tune: retune_ms = {retune_ms!r} gives a coefficient of {self.retune!r} per frame; it must lie in (0, 1]")
        self.retune_ms, self.hysteresis_cents = float(retune_ms), float(hysteresis_cents)
        self._strength = [float(s) for s in rows] if isinstance(strength, (list, tuple)) else float(strength)
        self._range(table, n)
        self.notes = torch.tensor(table, dtype=torch.float32)
        self.strength = torch.tensor(rows, dtype=torch.float32)
        if device is not None:
            self.notes = self.notes.to(gpu_device(device, "PitchSnap: the table lives on the GPU"))

    def _range(self, table, n):
        semitone = 2.0 ** (1.0 / 12.0)
        f_min, f_max = _f32(max(table[0] / semitone, 32.0)), _f32(table[n - 1] * semitone)
        if not (32.0 <= f_min <= f_max < math.inf):
            raise ValueError(f"tune: the table's range {f_min!r} .. {f_max!r} Hz: the highest note a semitone up must be finite and at least 32 Hz")
        self.f_min, self.f_max, self.n_notes = f_min, f_max, n

    def set_scale(self, key="C", scale="major", notes=None, a4=440.0, low=24, high=96):
        """Rebuild the table in place (the tensor a captured graph reads stays where it is).  f_min and f_max follow the new table: they
        are host values, so a stream whose range changed captures again."""
        table, n = note_table(key, scale, notes, a4, low, high)
        self._range(table, n)
        self.notes.copy_(torch.tensor(table, dtype=torch.float32))

    def bind(self, device, rows):
        """put the table and the strengths (one per row) on `device`: once, and again only for another device or number of rows"""
        if self.notes.device != device:
            self.notes = self.notes.to(device)
        if self.strength.device != device or self.strength.shape[0] != rows:
            given = self._strength
            if isinstance(given, list) and len(given) != rows:
                raise ValueError(f"tune: {len(given)} strengths for {rows} rows")
            self.strength = torch.tensor(given if isinstance(given, list) else [given] * rows, dtype=torch.float32, device=device)
        return self

    def params(self):
        """the host values a captured block bakes in"""
        return (self.hysteresis, self.retune, self.f_min, self.f_max)

    def settings(self):
        """the tvc_pitch_snap struct the library takes"""
        return PitchSnapSettings(*self.params())

    def __repr__(self):
        return f"PitchSnap({self.n_notes} notes, retune_ms={self.retune_ms:g}, hysteresis_cents={self.hysteresis_cents:g}, {self.f_min:g} .. {self.f_max:g} Hz)"


class SnapCarry:
    """The pitch correction's state of a set of streams that advance in lock step (tvc_tuned_convert_f32): a window advances by
    `hop_frames` = block_size / 480 frames per block, so what the correction holds behind frame hop_frames - 1 of one window is where
    frame 0 of the next starts.
      note  [S] int32   the note the stream is on (-1: none - unvoiced, out of range, fresh)
      ratio [S] fp32    the smoothed correction ratio there (1.0 with note -1)
    Whatever is written into them, the kernel takes a note only inside its table and a ratio only inside [2/3, 1.5].  Every window decodes an
    f0 of its own, so the state is a prior, not the run over any one tensor.  Every argument is checked before anything is allocated
    (ValueError)."""

    def __init__(self, n_streams, hop_frames, device=None):
        for x, name in ((n_streams, "n_streams"), (hop_frames, "hop_frames")):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1 or x > 0x7fffffff:
                raise ValueError(f"SnapCarry: {name} must be an integer >= 1, got {x!r}")
        self.n_streams, self.hop_frames = n_streams, hop_frames
        self.device = gpu_device(device, "SnapCarry: the state lives on the GPU (device='cpu' builds a carry no engine will take)", cpu_ok=True)
        stream_state.allocate(self, stream_state.SNAP_STATE, self.device)

    def params(self):
        """the host values a captured block bakes in"""
        return (self.hop_frames,)

    def reset(self, streams=None):
        """Start every stream, or the listed ones, without a note: in-place ops on the state tensors, so it works between replays of a
        captured graph (which reads them when it runs)."""
        stream_state.reset(self, stream_state.SNAP_STATE, streams)


def resolve_tune(tune):
    """convert's and the streams' `tune`: None -> None, a PitchSnap -> itself, 'A minor' / 'chromatic' -> PitchSnap(key, scale) with the
    defaults; ValueError for anything else, before any engine work"""
    if tune is None or isinstance(tune, PitchSnap):
        return tune
    if isinstance(tune, str):
        return PitchSnap(*parse_tune(tune))
    raise ValueError(f"tune: a feature_retrieval.PitchSnap or a string such as 'A minor', got {type(tune).__name__}")


def check_tune_carry(tune_carry, tune, B, frames):
    """convert's tune_carry (a SnapCarry or None) against the call, on the host"""
    if tune_carry is None:
        return None
    if not isinstance(tune_carry, SnapCarry):
        raise ValueError(f"tune_carry: a feature_retrieval.SnapCarry, got {type(tune_carry).__name__}")
    if tune is None:
        raise ValueError("tune_carry needs tune: the state it carries is the pitch correction's")
    if tune_carry.n_streams != B:
        raise ValueError(f"tune_carry: a carry of {tune_carry.n_streams} streams for a batch of {B}")
    if frames < tune_carry.hop_frames:
        raise ValueError(f"tune_carry: hop_frames = {tune_carry.hop_frames} must be at most the call's {frames} frames")
    return tune_carry


def check_stream_tune(tune, block_size):
    """a stream's `tune` on the host (ValueError, before anything is allocated) -> None or the PitchSnap"""
    tune = resolve_tune(tune)
    if tune is not None and block_size % 480:
        raise ValueError(f"tune: block_size = {block_size} is not a whole number of 480-sample frames (the correction's state travels from "
                         "window to window, so the window must advance by whole frames)")
    return tune


def add_tune_arguments(parser):
    """`--tune "KEY SCALE"` and the correction's settings for the entry scripts' parsers: absent is the call without it"""
    parser.add_argument("--tune", default=None, metavar='"KEY SCALE"',
                        help="pitch correction: snap the pitch the decoder plays to the notes of a scale, e.g. \"A minor\", \"C major\", chromatic "
                             f"(keys {' '.join(KEYS)}; scales {' '.join(SCALES)}).  The defaults are guesses: nobody has listened")
    parser.add_argument("--tune-notes", default=None, metavar="M,M,...", help="... or to an explicit list of MIDI note numbers (69 = A4)")
    for flag, what in (("--tune-a4", "the pitch of A4 in Hz (default 440)"), ("--tune-retune", "retune time in ms; 0 snaps at once and flattens vibrato (default 60)"),
                       ("--tune-strength", "share of the correction that is applied, 0 .. 1 (default 1)"),
                       ("--tune-hysteresis", "cents a pitch must pass the bound between two notes before it changes note, 0 .. 100 (default 25)")):
        parser.add_argument(flag, type=float, default=None, help=f"--tune: {what}.  Nobody has listened")


def tune_keywords(args, script):
    """what `--tune` and its settings add to the script's convert / stream keywords: nothing when absent, else {"tune": a PitchSnap} and
    one printed line; a setting without `--tune` / `--tune-notes`, or a refused one, ends the script"""
    flags = {"a4": "a4", "retune_ms": "retune", "strength": "strength", "hysteresis_cents": "hysteresis"}      # PitchSnap's keyword -> the flag's tail
    given = {k: getattr(args, "tune_" + a, None) for k, a in flags.items()}
    given = {k: v for k, v in given.items() if v is not None}
    tune, notes = getattr(args, "tune", None), getattr(args, "tune_notes", None)
    if tune is None and notes is None:
        if given:
            sys.exit(f"{script}: --tune-{flags[next(iter(given))]} belongs to --tune")
        return {}
    try:
        if notes is not None:
            if tune is not None:
                raise ValueError("tune: --tune and --tune-notes are two ways to give the table; give one")
            try:
                given["notes"] = [int(m) for m in notes.split(",")]
            except ValueError:
                raise ValueError(f"tune: --tune-notes takes MIDI numbers separated by commas, got {notes!r}") from None
        else:
            given["key"], given["scale"] = parse_tune(tune)
        snap = PitchSnap(**given)
    except ValueError as e:
        sys.exit(f"{script}: {e}")
    print(f"Correcting pitch: {snap!r} (untuned defaults: nobody has listened)")
    return {"tune": snap}


def resolve_f0_estimation(f0_estimation):
    """convert's f0_estimation: 'viterbi' -> PitchPath() with the defaults, a PitchPath -> itself, anything else (the reference's 'default',
    'fcpe', 'dio', 'harvest', ...) -> None: accepted and ignored exactly as in the reference"""
    if isinstance(f0_estimation, PitchPath):
        return f0_estimation
    return PitchPath() if isinstance(f0_estimation, str) and f0_estimation == "viterbi" else None


def add_f0_arguments(parser, choices=None):
    """`-f0-est` and the pitch path's five settings for the entry scripts' parsers.  `choices`: the script's own list of accepted names"""
    kw = {"choices": choices} if choices is not None else {}
    parser.add_argument("-f0-est", "--f0-estimation", default="default",
                        help="viterbi: decode the pitch logits as one path over each utterance (a stream: each window) instead of frame by "
                             "frame; every other name is accepted and ignored, as in the reference", **kw)
    for flag, typ, what in (("--f0-step", float, "cost per class of distance inside the band (default 0.5)"),
                            ("--f0-band", int, "classes a voiced frame may move at that cost, 0 .. 32; 48 are one octave (default 12)"),
                            ("--f0-jump", float, "cost of any longer move between voiced classes, >= band * step (default 12)"),
                            ("--f0-voicing", float, "cost of a move between unvoiced and voiced (default 3)"),
                            ("--f0-refine", int, "classes on each side of the path's that share the frequency, 0 .. 4 (default 2)")):
        parser.add_argument(flag, type=typ, default=None, help=f"-f0-est viterbi: {what}.  The defaults are guesses: nobody has listened")


def add_f0_carry_argument(parser):
    """`--f0-carry` for the entry scripts that stream"""
    parser.add_argument("--f0-carry", action="store_true",
                        help="-f0-est viterbi in a stream: carry the path's scores from block to block (an online Viterbi) instead of decoding "
                             "every window from a flat start; block_size must be whole 480-sample frames.  Nobody has listened")


def f0_carry_keywords(args, script):
    """what `--f0-carry` adds to the script's stream keywords: nothing when absent, else {"f0_carry": True} and one printed line; the flag
    without `-f0-est viterbi` ends the script"""
    if not getattr(args, "f0_carry", False):
        return {}
    if args.f0_estimation != "viterbi":
        sys.exit(f"{script}: --f0-carry belongs to -f0-est viterbi")
    print("Carrying the pitch path's scores from block to block (nobody has listened)")
    return {"f0_carry": True}


def f0_keywords(args, script):
    """what `-f0-est` and the --f0-* settings make of the script's f0_estimation keyword: the name as it was given, or with `viterbi` a
    PitchPath and one printed line; a setting without `-f0-est viterbi`, or a refused one, ends the script"""
    given = {k: getattr(args, "f0_" + k, None) for k in ("step", "band", "jump", "voicing", "refine")}
    given = {k: v for k, v in given.items() if v is not None}
    if args.f0_estimation != "viterbi":
        if given:
            sys.exit(f"{script}: --f0-{next(iter(given))} belongs to -f0-est viterbi")
        return args.f0_estimation
    try:
        path = PitchPath(**given)
    except ValueError as e:
        sys.exit(f"{script}: {e}")
    print(f"Decoding pitch as a path: {path!r} (untuned defaults: nobody has listened)")
    return path


def add_alpha_argument(parser):
    """`--alpha A` and `--protect P` for the entry scripts' parsers: absent (None) is the call without them"""
    parser.add_argument("--alpha", type=float, default=None,
                        help="keep this share of the source's own content features in the match (the reference's match_features alpha; RVC's "
                             "index rate is 1 - alpha); default: absent, the plain match")
    parser.add_argument("--protect", type=float, default=None,
                        help="raise that share on unvoiced frames (consonants, breaths, silence) to alpha + (1 - alpha) * P, by the f0 the "
                             "conversion decodes; voiced frames keep alpha.  1 - RVC's protect value; meant for 0 .. 1.  An untuned guess: nobody "
                             "has listened.  default: absent, the same share on every frame")


def alpha_keywords(args, script):
    """what `--alpha` / `--protect` add to the script's convert / stream call: nothing when they are absent (the call is today's), else
    {"alpha": A} / {"protect": P} and one printed line each; a non-finite value ends the script"""
    kw = {}
    if args.alpha is not None:
        if not math.isfinite(args.alpha):
            sys.exit(f"{script}: --alpha must be a finite number")
        print(f"Keeping {args.alpha:g} of the source's own content features (alpha; index rate {1 - args.alpha:g})")
        kw["alpha"] = float(args.alpha)
    protect = getattr(args, "protect", None)
    if protect is not None:
        if not math.isfinite(protect):
            sys.exit(f"{script}: --protect must be a finite number")
        print(f"Protecting unvoiced frames: their share of the source's own features rises by {protect:g} of what the match would take (protect)")
        kw["protect"] = float(protect)
    return kw


def add_match_weight_argument(parser):
    """`-k K` and `--match-width W` for the entry scripts' parsers: absent (None) is the call without them"""
    parser.add_argument("-k", "--neighbours", dest="k", type=int, default=None,
                        help="average the K nearest index rows of every frame (1 .. 4; the reference's match_features k); default: absent, "
                             "the four nearest with equal weight")
    parser.add_argument("--match-width", type=float, default=None,
                        help="weight neighbour e by clamp(1 - (s_0 - s_e) / W, 0, 1), s the cosine similarities: W in cosine units, >= 0 "
                             "(inf: equal weights, 0: the nearest row alone).  No value is suggested: nobody has listened.  default: absent")


def match_weight_keywords(args, script):
    """what `-k` / `--match-width` add to the script's convert / stream call: nothing when they are absent (the call is today's), else
    {"k": K} / {"match_width": W} and one printed line; a value outside its range ends the script"""
    kw = {}
    if args.k is not None:
        if not 1 <= args.k <= 4:
            sys.exit(f"{script}: -k must be 1 .. 4 (the fused match keeps four neighbours)")
        kw["k"] = int(args.k)
    if args.match_width is not None:
        if not args.match_width >= 0:
            sys.exit(f"{script}: --match-width must be >= 0 (cosine units; inf: equal weights)")
        kw["match_width"] = float(args.match_width)
    if kw:
        print(f"Weighted match: the {kw.get('k', 4)} nearest rows of every frame, similarity width {kw.get('match_width', math.inf):g}")
    return kw


def add_continuity_argument(parser):
    """`--continuity C` for the entry scripts' parsers: absent (None) is the call without it"""
    parser.add_argument("--continuity", type=float, default=None, metavar="C",
                        help="match along a path: choose the neighbour a frame's weights form around over the utterance as a whole, a neighbour "
                             "gaining C times its cosine to the neighbour chosen for the frame before (>= 0; needs a finite --match-width).  "
                             "No value is suggested: nobody has listened.  default: absent")


def continuity_keywords(args, script, so_far):
    """what `--continuity` adds to the script's convert / stream call (`so_far`: match_weight_keywords' result for the same arguments):
    nothing when it is absent (the call is today's), else {"continuity": C} and one printed line; a value outside its range, or one that
    could have no effect, ends the script"""
    if args.continuity is None:
        return {}
    if not args.continuity >= 0:
        sys.exit(f"{script}: --continuity must be >= 0")
    if args.continuity > 0 and not math.isfinite(so_far.get("match_width", math.inf)):
        sys.exit(f"{script}: --continuity needs a finite --match-width: under an infinite width every neighbour weighs 1 wherever the path goes")
    print(f"Match along a path: continuity {args.continuity:g}")
    return {"continuity": float(args.continuity)}


def gpu_device(device, sentence, cpu_ok=False):
    """where a stream stage's state lives: `device` (None: "cuda") as a torch.device, refused (ValueError: `sentence` - the stage's own words -
    and what was given) before anything is allocated when it is not a GPU that is there; cpu_ok: a CPU device passes"""
    device = torch.device(device if device is not None else "cuda")
    if not (torch.cuda.is_available() if device.type == "cuda" else cpu_ok):
        raise ValueError(f"{sentence}; got device {str(device)!r}" + ("" if torch.cuda.is_available() else " and there is no GPU here"))
    return device


class PitchTrack:
    """The pitch tracker of a set of streams that advance in lock step (tvc_pitch_track_f32 / tvc_convert_track_f32): the register a
    stream's automatic shift aims FROM is the lower median of its last `window_frames` voiced f0 values, kept on the device.
      ring [S, W] fp32   the last W voiced f0 values of each stream (a ring; unwritten slots are 0.0)
      count [S] int64    voiced frames appended since the last reset (write cursor count % W, fill min(count, W))
      auto [S] fp32      the automatic part of the shift applied in the latest block
    Per block the kernel appends the voiced frames among the `new_frames` columns that end `lag_frames` before the end of f0, and moves
    `auto` toward 12 log2(target / median) by at most `slew` semitones (per block; inf = at once).  Before `min_voiced` values are in the
    ring the automatic shift is 0.  Every argument is checked before anything is allocated (ValueError)."""

    def __init__(self, n_streams, new_frames, lag_frames=0, window_frames=1500, min_voiced=25, slew=float("inf"), device=None):
        def whole(x, name, lo, hi=None):
            if isinstance(x, bool) or not isinstance(x, int) or x < lo or (hi is not None and x > hi):
                raise ValueError(f"PitchTrack: {name} must be an integer {'>= ' + str(lo) if hi is None else 'in ' + str(lo) + ' ... ' + str(hi)}, got {x!r}")
            return x
        self.n_streams = whole(n_streams, "n_streams", 1)
        self.new_frames = whole(new_frames, "new_frames", 0, spec.PITCH_TRACK_MAX_NEW)
        self.lag_frames = whole(lag_frames, "lag_frames", 0)
        self.window_frames = whole(window_frames, "window_frames", 1, spec.PITCH_TRACK_MAX_WINDOW)
        self.min_voiced = whole(min_voiced, "min_voiced", 1, 0x7fffffff)
        if isinstance(slew, bool) or not isinstance(slew, (int, float)) or not float(slew) >= 0.0:
            raise ValueError(f"PitchTrack: slew must be >= 0 semitones per block (inf: no limit), got {slew!r}")
        self.slew = float(slew)
        self.device = gpu_device(device, "PitchTrack: the state lives on the GPU (device='cpu' builds a tracker no engine will take)", cpu_ok=True)
        stream_state.allocate(self, stream_state.TRACK_STATE, self.device)

    def columns(self, T):
        """the tracked columns [start, start + new_frames) of an f0 of T frames; ValueError when they do not fit"""
        start = T - self.lag_frames - self.new_frames
        if start < 0:
            raise ValueError(f"track: {self.new_frames} new frames ending {self.lag_frames} before the end do not fit T = {T} frames")
        return start, self.new_frames

    def params(self):
        """the host values a captured block bakes in"""
        return (self.new_frames, self.lag_frames, self.window_frames, self.min_voiced, self.slew)

    def reset(self, streams=None):
        """Forget the history of every stream, or of the listed ones: in-place ops on the state tensors, so it works between replays of a
        captured graph (which reads them when it runs)."""
        stream_state.reset(self, stream_state.TRACK_STATE, streams)

    def register(self):
        """the streams' registers as they stand: PitchRegister(median_hz [S], voiced [S] = the fill)"""
        return pitch_register(self.ring)


def add_auto_pitch_argument(parser):
    """`--auto-pitch` for infer.py's parser: shift every file so that its median f0 lands on the target's (-p stays, as the offset)."""
    parser.add_argument("--auto-pitch", action="store_true",
                        help="move every file's median f0 onto the target speaker's (from the index's .f0.pt sidecar, or the -t recording); -p is added on top")


def target_form(tgt):
    """How convert reads its target -> ("blend" | "table" | "shared", the index tensors it consists of): a Blend; one index per row (a list /
    tuple of tensors, or a 3-D tensor of more than one row); else one index shared by every row (not shape-checked on the host)."""
    if isinstance(tgt, Blend):
        return "blend", tgt.term_tensors()
    if isinstance(tgt, (list, tuple)):
        return "table", list(tgt)
    if isinstance(tgt, torch.Tensor) and tgt.dim() == 3 and tgt.shape[0] != 1:
        return "table", [tgt]
    return "shared", [tgt]


def check_references(tgt, B=None):
    """Shape check of a multi-index target, on the host (no engine, no device work): a [B, 768, N] tensor or a list of B [1, 768, N_b]
    tensors (fp32 or fp16).  Returns the number of indices; raises ValueError when the form is malformed or B does not match."""
    if isinstance(tgt, torch.Tensor):
        if tgt.dim() != 3 or tgt.shape[1] != 768 or tgt.shape[0] < 1 or tgt.shape[2] < 4:
            raise ValueError(f"target indices: a [B, 768, N >= 4] tensor, got {tuple(tgt.shape)}")
        n = tgt.shape[0]
    elif isinstance(tgt, (list, tuple)):
        if not tgt:
            raise ValueError("target indices: an empty list")
        for i, t in enumerate(tgt):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != 1 or t.shape[1] != 768 or t.shape[2] < 4:
                raise ValueError(f"target indices: element {i} must be a [1, 768, N >= 4] tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.dtype not in (torch.float32, torch.float16):
                raise ValueError(f"target indices: element {i} must be fp32 or fp16, got {t.dtype}")
        n = len(tgt)
    else:
        raise ValueError(f"target indices: a tensor or a list of tensors, got {type(tgt).__name__}")
    if B is not None and n != B:
        raise ValueError(f"{n} target indices for a batch of {B}")
    return n


BLEND_MAX = spec.BLEND_MAX      # terms per row (TVC_BLEND_MAX)


def _term_rows(term, m):
    """rows a blend term speaks for: None = one shared index for every row ([1, 768, N]), else B"""
    if not isinstance(term, (torch.Tensor, list, tuple)):
        raise ValueError(f"blend term {m}: a [1 or B, 768, N] tensor or a list of [1, 768, N_b] tensors, got {type(term).__name__}")
    n = check_references(term)
    if isinstance(term, torch.Tensor):
        if term.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"blend term {m} must be fp32 or fp16, got {term.dtype}")
        return None if n == 1 else n
    return n


def check_blend(terms, weights, B=None):
    """Shape check of a blend, on the host (no engine, no device work; beside check_references): `terms` = 1 ... 4 targets, each in any form
    `convert` takes as tgt (a shared [1, 768, N], a [B, 768, N] tensor or a list of B [1, 768, N_b], fp32 or fp16); `weights` = M floats, B rows
    of M floats, or a tensor [M] or [B, M].  Returns (M, rows) - rows = the batch the blend is made for, None when every term is shared and the weights are
    per term (it then fits any batch); raises ValueError when the form is malformed or the row counts disagree (with each other or with B)."""
    if not isinstance(terms, (list, tuple)):
        raise ValueError(f"blend terms: a list of targets, got {type(terms).__name__}")
    M = len(terms)
    if not 1 <= M <= BLEND_MAX:
        raise ValueError(f"a blend takes 1 ... {BLEND_MAX} terms, got {M}")
    rows = B
    for m, t in enumerate(terms):
        n = _term_rows(t, m)
        if n is not None:
            if rows is not None and n != rows:
                raise ValueError(f"blend term {m} holds {n} indices for a batch of {rows}")
            rows = n
    if not isinstance(weights, torch.Tensor):      # floats, or nested rows of floats
        try:
            weights = torch.as_tensor(weights, dtype=torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"blend weights: {M} floats, or a tensor [M] or [B, M], got {type(weights).__name__}") from None
    if weights.dim() == 1:
        ok = weights.shape[0] == M
    else:
        ok = weights.dim() == 2 and weights.shape[1] == M and (rows is None or weights.shape[0] == rows)
        if ok:
            rows = weights.shape[0]
    if not ok:
        raise ValueError(f"blend weights: [M = {M}] or [B{'' if rows is None else ' = ' + str(rows)}, M = {M}], got {tuple(weights.shape)}")
    if not weights.dtype.is_floating_point:
        raise ValueError(f"blend weights must be floating point, got {weights.dtype}")
    return M, rows


class Blend:
    """A weighted blend of speaker indices as a conversion target: out = w_0 * match(src, terms[0]) + w_1 * match(src, terms[1]) + ...
    (the kNN-VC voice morph; weights may be negative or zero and are not normalised).  `terms` and `weights` as check_blend takes them.
    A weights tensor that is already on the device, fp32, contiguous and [B, M] is used IN PLACE: the kernels read it when they run, so
    `blend.weights.copy_(...)` takes effect on the next call - and on the next replay of a captured stream graph, without a new capture.
    Anything else is expanded once into a device tensor the object owns (`.weights`; made at construction when the rows and the device are
    known, else at the first use).  The terms' prepared blobs ride on the caller's tensors (prepare_reference / prepare_references): nothing
    is prepared twice.  `terms` is a plain list: replacing an entry takes effect on the next call."""

    def __init__(self, terms, weights):
        self.M, self.rows = check_blend(terms, weights)
        self.terms = list(terms)
        self._given = weights
        self.weights = None
        live = (isinstance(weights, torch.Tensor) and weights.dim() == 2 and weights.device.type == "cuda" and weights.dtype == torch.float32
                and weights.is_contiguous())
        if live:
            self.weights = weights
        elif self.rows is not None:
            first = self.terms[0][0] if isinstance(self.terms[0], (list, tuple)) else self.terms[0]
            dev = weights.device if isinstance(weights, torch.Tensor) and weights.device.type == "cuda" else first.device
            if dev.type == "cuda":
                self.weights = self._expand(self.rows, dev)

    def _expand(self, B, device):
        w = torch.as_tensor(self._given, dtype=torch.float32).detach().to("cpu")
        if w.dim() == 1:
            w = w[None].expand(B, self.M)
        return w.contiguous().to(device)

    def term_tensors(self):
        """every index tensor the blend holds, in term order (what a captured graph keys on)"""
        out = []
        for t in self.terms:
            out.extend(t if isinstance(t, (list, tuple)) else [t])
        return out

    def resolve(self, B, device, to_device=None):
        """-> (blobs [B * M], Ns [B * M], weights [B, M] on `device`): the row-major tables of a batch of B rows.  Host checks first;
        `to_device` (optional) maps every index tensor to the device (Generator._input_device)."""
        check_blend(self.terms, self._given, B)
        device = torch.device(device)
        w = self.weights
        if w is None or w.shape[0] != B or w.device != device:
            if w is not None and w is self._given:
                raise ValueError(f"blend weights live on {w.device}, the batch on {device}")
            w = self.weights = self._expand(B, device)
        move = to_device if to_device is not None else (lambda t: t)
        cols = []
        for t in self.terms:
            if isinstance(t, (list, tuple)):
                cols.append(prepare_references([move(x) for x in t]))
            elif t.shape[0] == 1:
                blob, n = prepare_reference(move(t))
                cols.append(([blob] * B, [n] * B))
            else:
                cols.append(prepare_references(move(t)))
        blobs = [cols[m][0][b] for b in range(B) for m in range(self.M)]
        ns = [cols[m][1][b] for b in range(B) for m in range(self.M)]
        return blobs, ns, w


def parse_blend(items):
    """The entry scripts' `--blend PATH=W [PATH=W ...]`: 1 ... 4 index files and their weights -> (paths, weights).  ValueError for a
    missing or malformed weight, an empty path or too many entries."""
    items = list(items)
    if not 1 <= len(items) <= BLEND_MAX:
        raise ValueError(f"1 ... {BLEND_MAX} PATH=WEIGHT entries, got {len(items)}")
    paths, weights = [], []
    for it in items:
        path, sep, w = str(it).rpartition("=")
        if not sep or not path:
            raise ValueError(f"{it!r}: expected PATH=WEIGHT")
        try:
            weights.append(float(w))
        except ValueError:
            raise ValueError(f"{it!r}: the weight {w!r} is not a number") from None
        paths.append(path)
    return paths, weights


def add_blend_argument(parser):
    """`--blend PATH=W [PATH=W ...]` for an entry script's argparse parser: args.blend = (paths, weights) or None; a malformed list is
    refused at parse time (parse_blend)."""
    import argparse

    class BlendArg(argparse.Action):
        def __call__(self, parser_, namespace, values, option_string=None):
            try:
                setattr(namespace, self.dest, parse_blend(values))
            except ValueError as e:
                parser_.error(f"--blend: {e}")

    parser.add_argument("--blend", nargs="+", metavar="PATH=W", default=None, action=BlendArg,
                        help="convert toward a weighted blend of up to four index files (index.pt=WEIGHT ...) instead of -idx / -t")


@torch.no_grad()
def match_features_blend(source, blend, return_indices=False):
    """source [B, 768, T], blend = Blend(terms, weights) -> [B, 768, T] = sum_m w[b][m] * match_features(source[b], term m's index of row b)
    in term order, one call (tvc_knn_match_blend_f32; k = 4, 'cos'); return_indices: also [M, B, T, 4], each term's own search."""
    eng = default_engine(source.device)
    blobs, ns, w = blend.resolve(source.shape[0], source.device)
    return eng.knn_match_blend(source, blobs, ns, w, want_indices=return_indices)


def prepare_references(tgt):
    """One prepared index per row: `tgt` is a [B, 768, N] tensor (the reference's form) or a list of B [1, 768, N_b] tensors (speakers with
    different amounts of target audio, fp32 or fp16 storage) -> (blobs [B], Ns [B]).  Cached on the tensor object(s) the caller holds,
    keyed by their version and device like prepare_reference - never on slices, so a second call prepares nothing."""
    check_references(tgt)
    if isinstance(tgt, (list, tuple)):
        pairs = [prepare_reference(t) for t in tgt]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    hit = getattr(tgt, "_tvc_prepared_rows", None)
    if hit is not None and hit[0] == tgt._version and hit[1] == str(tgt.device):
        return hit[2], hit[3]
    eng = default_engine(tgt.device)
    pairs = [eng.knn_prepare(tgt[b:b + 1]) for b in range(tgt.shape[0])]
    blobs, ns = [p[0] for p in pairs], [p[1] for p in pairs]
    try:
        tgt._tvc_prepared_rows = (tgt._version, str(tgt.device), blobs, ns)
    except Exception:
        pass
    return blobs, ns


@torch.no_grad()
def match_features(source, reference, k=4, alpha=0.0, metrics="cos", return_indices=False):
    """source [B, C, T], reference [B or 1, C, N] -> [B, C, T] (mean of the k nearest index vectors under `metrics` in
    {'cos', 'IP', 'L2'}, k = 1 ... 8, blended with the input by alpha): the reference's signature, feature_retrieval.py:15."""
    if reference.device != source.device:
        reference = reference.to(source.device)
    eng = default_engine(source.device)
    B = source.shape[0]
    if k != 4 or metrics != "cos":
        # every other argument of the reference's signature: plain fp32 on the raw index (csrc/knn_general.hip); the inference path's k = 4 /
        # 'cos' below runs the prepared-index search on the matrix pipe
        if reference.shape[0] not in (1, B):
            raise RuntimeError(f"batch of reference ({reference.shape[0]}) must be 1 or match source ({B})")
        if reference.shape[0] == 1:
            res = eng.knn_match_general(source, reference[0].float(), k, metrics, want_indices=True)
        else:
            parts = [eng.knn_match_general(source[b:b + 1], reference[b].float(), k, metrics, want_indices=True) for b in range(B)]
            res = (torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0))
        out, idx = res
        if alpha != 0.0:
            out = out * (1 - alpha) + source * alpha
        return (out, idx) if return_indices else out
    if reference.shape[0] == 1:
        blob, n = prepare_reference(reference)
        res = eng.knn_match(source, blob, n, want_indices=return_indices)
        out, idx = res if return_indices else (res, None)
    elif reference.shape[0] == B:
        blobs, ns = prepare_references(reference)      # one index per utterance, one call (tvc_knn_match_multi_f32)
        res = eng.knn_match_multi(source, blobs, ns, want_indices=return_indices)
        out, idx = res if return_indices else (res, None)
    else:
        raise RuntimeError(f"batch of reference ({reference.shape[0]}) must be 1 or match source ({B})")
    if alpha != 0.0:
        out = out * (1 - alpha) + source * alpha
    return (out, idx) if return_indices else out
