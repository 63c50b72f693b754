"""Real-time wrapper: rolling input buffer, full convert per block, SOLA alignment and cross-fade
(reference module/infer/stream.py:30-96).  `StreamInfer` is the reference's single-stream class;
`BatchedStreamInfer` runs S independent streams through one batched convert + one SOLA launch with
the lag arg-max kept on the device."""
import numpy as np
import torch

from ...engine import pitch_shifts
from ..tinyvc.feature_retrieval import PitchTrack, resolve_auto_pitch, target_form
from .generator import Generator


def _fade_windows(crossfade_size, device):
    # stream.py:61-62, computed on the host exactly as the reference does, then uploaded
    fade_in = torch.sin(np.pi * torch.arange(0, 1, 1 / crossfade_size) / 2) ** 2
    return fade_in.to(device), (1 - fade_in).to(device)


class BatchedStreamInfer:
    """`target`: one index for every stream ([1, 768, N]) or one per stream ([S, 768, N], or a list of S [1, 768, N_s] tensors), prepared
    once and cached on those tensors - or a feature_retrieval.Blend of several (its weights are read on the device when a block runs:
    `blend.weights.copy_(...)` between blocks moves the mix without a new graph capture); `pitch_shift`: a float or one per stream.
    `auto_pitch` (convert's: True, a register in Hz, or a [S] / [1] device tensor that is read when a block runs): every block moves each
    stream's register - the lower median of its last voiced frames, tracked on the device by `pitch_track` (a feature_retrieval.PitchTrack;
    built in init_buffer when not given: the block's own frames, last_dilay_size before the end of the buffer, are the new ones) - onto
    the target's; `pitch_shift` is the offset on top and `last_pitch_shift` [S] the shift the latest block applied, on the device."""

    def __init__(self, generator: Generator, n_streams=1, target=None, pitch_shift=0., device=None,
                 block_size=1920, extra_size=0, use_phase_vocoder=False, f0_estimation="default", use_graph=False, auto_pitch=None, pitch_track=None):
        self.auto_pitch = auto_pitch if auto_pitch is not False else None
        self.pitch_track = pitch_track
        self._own_track = pitch_track is None
        if pitch_track is not None and self.auto_pitch is None:
            raise ValueError("pitch_track needs auto_pitch: the tracker finds the register the automatic shift starts from")
        if self.auto_pitch is not None and block_size % 480:
            raise ValueError(f"auto_pitch: block_size = {block_size} is not a whole number of 480-sample frames")
        self.last_pitch_shift = None
        self.generator = generator
        self.n_streams = n_streams
        self.target = target
        self.pitch_shift = pitch_shift
        self.device = torch.device(device) if device is not None else generator._module_device()
        self.block_size = block_size
        self.extra_size = extra_size
        self.sola_search_size = 1920
        self.last_dilay_size = 3840          # (sic) the reference's attribute name, stream.py:49
        self.crossfade_size = 1920
        self.use_phase_vocoder = use_phase_vocoder
        self.f0_estimation = f0_estimation
        self.input_size = max(self.block_size + self.crossfade_size + self.sola_search_size + 2 * self.last_dilay_size,
                              self.block_size + self.extra_size)
        self.last_shift = None
        # use_graph: after two eager warm-up blocks the whole per-block pipeline (buffer roll, noise draw,
        # convert, SOLA) is captured once into a HIP graph and replayed per block: ~170 launches become one.
        self.use_graph = use_graph
        self._graph = None
        self._calls = 0

    def init_buffer(self):
        self.fade_in_window, self.fade_out_window = _fade_windows(self.crossfade_size, self.device)
        self.input_wav = torch.zeros(self.n_streams, self.input_size, device=self.device)
        self.sola_buffer = torch.zeros(self.n_streams, self.crossfade_size, device=self.device)
        self._graph = None
        self._calls = 0
        if self.auto_pitch is not None:
            if self._own_track:      # the block's own frames: they have their full right context and are the audio about to be played
                self.pitch_track = PitchTrack(self.n_streams, self.block_size // 480, self.last_dilay_size // 480, device=self.device)
            self.pitch_track.reset()

    def _step(self, blocks, noise_angle):
        # torch.roll + slice assignment of the reference (stream.py:69-70), in place on a fixed buffer, one launch
        self.generator.engine(self.device).stream_push(self.input_wav, blocks)
        if noise_angle is None and self.use_graph:
            # a captured step bakes kernel arguments in: the library's seeded draw would replay ONE seed for every block.  torch's
            # generator is graph-safe (its offset advances per replay), so the graph path keeps the reference's torch.rand draw
            from ..tinyvc import Decoder
            noise_angle = Decoder.draw_noise_angle(self.n_streams, self.input_size // 480, self.device)
        pshift = None
        if self.auto_pitch is None:
            y = self.generator.convert(self.input_wav, self.target, self.pitch_shift, device=self.device,
                                       f0_estimation=self.f0_estimation, noise_angle=noise_angle)
        else:
            y, pshift = self.generator.convert(self.input_wav, self.target, self.pitch_shift, device=self.device, f0_estimation=self.f0_estimation,
                                               noise_angle=noise_angle, auto_pitch=self.auto_pitch, return_shift=True, track=self.pitch_track)
        eng = self.generator.engine(self.device)
        return eng.sola(y, self.sola_buffer, self.fade_in_window, self.block_size,
                        self.use_phase_vocoder, want_shift=True) + (pshift,)

    def _graph_key(self):
        """Everything a captured step bakes in as raw device pointers: the packed weights (re-packed - and the old arena
        freed - when a parameter changes), the engine's scratch workspace (re-allocated when another call needs a bigger
        one), the prepared index riding on `target`, plus the scalars captured by value.  With auto_pitch also the
        tracker's three state tensors (where they live) and its host parameters, and WHERE the target registers live - not their values,
        nor the ring's or `auto`'s: the kernels read those at replay, so a reset(), registers.copy_(...) or a stream's history advancing
        keeps the graph."""
        eng = self.generator.engine(self.device)          # re-packs the weights first if a parameter changed
        ws = eng._ws
        form, tgts = target_form(self.target)      # every blob's tensor
        wkey = 0
        if form == "blend":      # WHERE the weights live - not their version or values: the kernels read them at replay
            wkey = self.target.resolve(self.n_streams, self.device, self.generator._input_device)[2].data_ptr()
        shift, shifts = pitch_shifts(self.pitch_shift, self.n_streams)
        shifts = shift if shifts is None else tuple(shifts)
        tkey = ()
        if self.auto_pitch is not None:
            regs = resolve_auto_pitch(self.auto_pitch, self.target, self.n_streams)
            tr = self.pitch_track
            tkey = (regs if isinstance(regs, float) else tuple(r.data_ptr() for r in regs), tr.ring.data_ptr(), tr.count.data_ptr(), tr.auto.data_ptr(),
                    tr.params())
        return (eng.weights_key, ws.data_ptr() if ws is not None else 0, ws.numel() if ws is not None else 0,
                tuple((id(t), t._version, t.data_ptr()) for t in tgts), wkey, shifts, bool(self.use_phase_vocoder)) + tkey

    @torch.no_grad()
    def audio_callback(self, blocks, noise_angle=None):
        """blocks [S, block_size] -> converted blocks [S, block_size]."""
        blocks = blocks.to(self.device)
        self._calls += 1
        if not self.use_graph or self._calls <= 2:
            out, self.last_shift, self.last_pitch_shift = self._step(blocks, noise_angle)
            return out
        key = self._graph_key()
        if self._graph is not None and key != self._graph[0]:
            self._graph = None        # stale pointers inside the captured graphs: drop them and capture again
        if self._graph is None:
            self._graph = (key, {})
            self._g_in = torch.zeros(self.n_streams, self.block_size, device=self.device)
            self._g_angle = torch.zeros(self.n_streams, 961, self.input_size // 480, device=self.device)
        inject = noise_angle is not None      # injected phases replay from a static buffer; otherwise the draw is part of the graph
        graphs = self._graph[1]
        if inject not in graphs:
            self._g_in.copy_(blocks)
            if inject:
                self._g_angle.copy_(noise_angle)
            # capture changes no state: the buffer roll, convert and SOLA are recorded, not run
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                res = self._step(self._g_in, self._g_angle if inject else None)
            graphs[inject] = (g, res)
            if self._graph_key() != key:      # the capture itself grew the workspace: what it recorded is already stale
                self._graph = None
                out, self.last_shift, self.last_pitch_shift = self._step(blocks, noise_angle)
                return out
        self._g_in.copy_(blocks)
        if inject:
            self._g_angle.copy_(noise_angle)
        g, (g_out, g_shift, g_pshift) = graphs[inject]
        g.replay()
        self.last_shift, self.last_pitch_shift = g_shift, g_pshift
        return g_out.clone()


class StreamInfer(BatchedStreamInfer):
    """Single stream with the reference's constructor and 1-D buffers (stream.py:31-57)."""

    def __init__(self, generator: Generator, target=None, pitch_shift=0., device=torch.device("cpu"),
                 block_size=1920, extra_size=0, use_phase_vocoder=False, f0_estimation="default", use_graph=False, auto_pitch=None, pitch_track=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            dev = generator._module_device()     # the reference defaults to CPU; there is no CPU path here
        super().__init__(generator, 1, target, pitch_shift, dev, block_size, extra_size, use_phase_vocoder, f0_estimation, use_graph, auto_pitch, pitch_track)

    @torch.no_grad()
    def audio_callback(self, block, noise_angle=None):
        """block [block_size] -> converted block [block_size] (stream.py:68-96)."""
        return super().audio_callback(block[None], noise_angle)[0]
