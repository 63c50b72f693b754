"""The stream stages' device state against its declaration (tinyvc_amd.stream_state): the real stage objects own exactly the tensors their
tables list, a captured block's key follows where every one of them lives (and nothing they hold), and a stage built for other streams is
refused at init_buffer whichever stage it is.  No audio is converted and no graph captured there: everything is host work on a stream
set that has every stage.

The last test converts: a stream's state lives in the declared tensors and NOWHERE else - nothing survives from block to block in the
engine's workspace.  Two streams get the same blocks; before every block of one, the workspace is overwritten in place with a fill word of
tests/helpers_workspace.py (the pointer stays, so a captured graph stays valid), and the outputs are equal bit for bit, eager and replayed."""
import pytest
import torch

import helpers_workspace as W
from helpers import state_dicts
from tinyvc_amd import stream_state, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 3      # a reset row with a neighbour on either side
GEOM = dict(block_size=480, crossfade_size=240, sola_search_size=240, last_delay_size=480, extra_size=3840)


@pytest.fixture(scope="module")
def stream():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import BatchedStreamInfer, Generator, StreamDenoise, StreamDoor, StreamGate
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    from tinyvc_amd.module.tinyvc.feature_retrieval import PitchTrack
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    st = BatchedStreamInfer(Generator(enc, dec).to(DEV), n_streams=S, target=synth.synth_index(1000, seed=2).to(DEV), device=torch.device(DEV),
                            door=StreamDoor(S, 48000, 48000, 480, device=DEV), denoise=StreamDenoise(S, 480, hop=160, device=DEV),
                            gate=StreamGate(S, 480, hold_size=240, attack_size=240, release_size=480, lookahead_size=480, device=DEV),
                            auto_pitch=150.0, pitch_track=PitchTrack(S, 1, 1, window_frames=8, min_voiced=1, device=DEV), alpha=0.25, **GEOM)
    st.init_buffer()
    return st


def _stages(st):
    stages = st._stages()
    assert [(name, table) for name, _, table in stages] == [("track", stream_state.TRACK_STATE), ("door", stream_state.DOOR_STATE),
                                                            ("denoise", stream_state.DENOISE_STATE), ("gate", stream_state.GATE_STATE)]
    assert [stage for _, stage, _ in stages] == [st.pitch_track, st.door, st.denoise, st.gate]
    return stages


def test_no_stage_owns_a_tensor_its_table_does_not_list(stream):
    """what connects "allocated" to "checked, reset and keyed": a tensor a stage class adds without declaring it fails here"""
    for name, stage, table in _stages(stream):
        assert {k for k, v in vars(stage).items() if isinstance(v, torch.Tensor)} == {f.name for f in table}, name


def test_the_graph_key_follows_where_every_declared_tensor_lives(stream):
    key = stream._graph_key()
    assert stream._graph_key() == key
    for name, stage, table in _stages(stream):
        for f in table:
            home = getattr(stage, f.name)
            setattr(stage, f.name, home.clone())      # the same values at another address: a captured graph would read the old one
            assert stream._graph_key() != key, f"{name}.{f.name} moved and the key did not"
            setattr(stage, f.name, home)
            assert stream._graph_key() == key, f"{name}.{f.name}"
            # values never count: the kernels read them at replay
            home.fill_(3)
            home.copy_(torch.ones_like(home))
            assert stream._graph_key() == key, f"{name}.{f.name}: a value went into the key"
        stage.reset()
        stage.reset([1])
        assert stream._graph_key() == key, f"{name}.reset() changed the key"
    home = stream.alpha
    stream.alpha = home.clone()
    assert stream._graph_key() != key
    stream.alpha = home
    home.fill_(0.5)
    assert stream._graph_key() == key


@pytest.mark.parametrize("stage, attr, value", [("pitch_track", "min_voiced", 2), ("door", "output_gain", -3.0), ("denoise", "warm", 7), ("gate", "range_db", -20.0)])
def test_a_host_parameter_changes_the_key(stream, stage, attr, value):
    key = stream._graph_key()
    obj = getattr(stream, stage)
    old = getattr(obj, attr)
    assert old != value
    setattr(obj, attr, value)
    try:
        assert stream._graph_key() != key, f"{stage}.{attr} is baked into a captured block and not in its key"
    finally:
        setattr(obj, attr, old)
    assert stream._graph_key() == key


def test_a_foreign_door_is_met_at_init_buffer(stream):
    """attributes are plain: a door put in after construction is checked like a gate or a suppressor, before anything is allocated"""
    from tinyvc_amd.module.infer import StreamDoor
    own, window = stream.door, stream.input_wav
    stream.door = StreamDoor(2, 48000, 48000, 480, device=DEV)
    try:
        with pytest.raises(ValueError, match="door: built for 2 streams of 480-sample blocks, the streams are 3 of 480"):
            stream.init_buffer()
        assert stream.input_wav is window, "refused after the buffers were replaced"
    finally:
        stream.door = own
    stream.init_buffer()


# ---- nothing survives in the workspace from block to block ----------------------------------------------------------------------------------------
S2, WARM, MORE = 2, 2, 4      # two eager warm-up blocks (what a captured stream runs before it captures), then four more


@pytest.fixture(scope="module")
def converting():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    tgt = [synth.synth_index(300, seed=21).to(DEV), synth.synth_index(4097, seed=22).to(DEV).half()]      # the exact and the two-stage search
    blocks = (synth.synth_wave(S2, (WARM + MORE) * 480, seed=31) * 0.9).view(S2, WARM + MORE, 480).to(DEV)
    angles = [synth.synth_angle(S2, 9, 900 + i).to(DEV) for i in range(WARM + MORE)]
    return Generator(enc, dec).to(DEV), tgt, blocks, angles


def _fullest(gen, tgt, use_graph):
    """the fullest stream this module builds cheaply, at the smallest block geometry of the stream tests (a window of nine frames)"""
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamGate, StreamLimiter
    st = BatchedStreamInfer(gen, n_streams=S2, target=tgt, pitch_shift=[0.0, 2.0], device=torch.device(DEV), use_graph=use_graph, f0_estimation="viterbi",
                            f0_carry=True, alpha=0.25, protect=0.5,
                            gate=StreamGate(S2, 480, hold_size=240, attack_size=240, release_size=480, lookahead_size=480, device=DEV),
                            limiter=StreamLimiter(S2, 480, ceiling_db=-12.0, device=DEV), **GEOM)
    st.init_buffer()
    assert [name for name, _s, _t in st._stages()] == ["carry", "gate", "limiter"]
    return st


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_nothing_survives_in_the_workspace_from_block_to_block(converting, use_graph):
    gen, tgt, blocks, angles = converting
    plain, poisoned = _fullest(gen, tgt, use_graph), _fullest(gen, tgt, use_graph)
    eng = gen.engine(torch.device(DEV))
    captured = None
    for i in range(WARM + MORE):
        a = plain.audio_callback(blocks[:, i], noise_angle=angles[i]).clone()
        a_shift = plain.last_shift.clone()
        word = W.FILLS[i % len(W.FILLS)]
        where = eng._ws.data_ptr()
        W.fill_words(eng._ws, word)      # in place, on the stream the block runs on: the whole buffer, the 4096 bytes behind the peak too
        b = poisoned.audio_callback(blocks[:, i], noise_angle=angles[i]).clone()
        assert eng._ws.data_ptr() == where, "the workspace moved: the fill before this block went somewhere else"
        what = f"block {i + 1} behind a workspace of {word:#010x}"
        W.assert_same_bits((b, poisoned.last_shift), (a, a_shift), what)
        for (name, sa, table), (_n, sb, _t) in zip(plain._stages(), poisoned._stages()):
            W.assert_same_bits([getattr(sb, f.name) for f in table], [getattr(sa, f.name) for f in table], f"{what}: the state of {name}")
        if use_graph and i == WARM:      # captured at the first block behind the warm-up
            captured = poisoned._graph[0], poisoned._graph[1][True][0]
        if use_graph and i > WARM:
            assert poisoned._graph is not None and poisoned._graph[0] == captured[0] and poisoned._graph[1][True][0] is captured[1], \
                f"{what}: the graph was captured again"
    assert bool(a.abs().max() > 0), "silence: the comparison shows nothing"
    if use_graph:
        assert captured is not None and plain._graph is not None
    print(f"[ws] stream {'graph' if use_graph else 'eager'} (carry, alpha, protect, gate, limiter): the engine's {eng._ws.numel()} workspace bytes overwritten in place "
          f"before each of {WARM + MORE} blocks, fills cycling through {len(W.FILLS)}, outputs and state equal the untouched stream's"
          f"{', one capture' if use_graph else ''}")
