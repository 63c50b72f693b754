"""The stream stages' device state against its declaration (tinyvc_amd.stream_state): the real stage objects own exactly the tensors their
tables list, a captured block's key follows where every one of them lives (and nothing they hold), and a stage built for other streams is
refused at init_buffer whichever stage it is.  No audio is converted and no graph captured: everything here is host work on a stream
set that has every stage."""
import pytest
import torch

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
