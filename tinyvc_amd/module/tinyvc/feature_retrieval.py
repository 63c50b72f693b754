"""kNN-VC feature matching (reference module/tinyvc/feature_retrieval.py:15-33) on the streamed
top-k kernel of csrc/knn.hip."""
import torch

from ...engine import default_engine


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
    ssl, _f0, pre = generator.encode_packed(wf, lengths)
    cols = index_columns([pre[b + 1] - pre[b] for b in range(len(pre) - 1)], stride, size, perm)
    return index_from_columns(generator.engine(ssl.device), ssl, cols, half)


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
