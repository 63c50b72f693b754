"""The streaming door on the device (tvc_stream_resample; Engine.stream_resample, module.infer.StreamDoor, BatchedStreamInfer(door=...),
infer_streaming.py --resample).

The door has an exact definition, so everything here is bit for bit: for every prefix of a stream, the blocks emitted so far are the first
samples of the offline resampler (Engine.resample) applied to G * orig zeros followed by that prefix, and the state is the last `hist`
samples of zeros ++ input.  The int16 forms equal the fp32 door composed with the plain conversions, streams of one launch do not see each
other, and a stream served through a door equals the chain built from offline pieces only; a captured graph equals eager and survives a
reset and the history advancing without a new capture."""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import state_dicts
from tinyvc_amd import audio_io, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 3
PAIRS = [(48000, 24000), (44100, 24000), (16000, 24000), (8000, 24000), (24000, 48000), (24000, 44100), (24000, 8000)]
N_BLOCKS = 7
POISON = 1e30


def _engine():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.engine import default_engine
    return default_engine(torch.device(DEV))


def _bits(x):
    x = torch.as_tensor(x).cpu().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    """bit for bit (torch.equal would call -0.0 and 0.0 equal and a NaN unequal to itself)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _terms(in_freq, out_freq):
    g = math.gcd(in_freq, out_freq)
    return in_freq // g, out_freq // g


def _zeros_in_front(eng, in_freq, out_freq, n_in):
    """G * orig: the zeros the definition puts in front of a stream (G = delay / new)"""
    orig, new = _terms(in_freq, out_freq)
    _, _, delay = eng.stream_resample_geometry(in_freq, out_freq, n_in)
    assert delay % new == 0
    return delay // new * orig


def _offline(eng, x, in_freq, out_freq, n_in, n_total):
    """the definition: the first n_total samples of resample(G * orig zeros ++ x)"""
    z = _zeros_in_front(eng, in_freq, out_freq, n_in)
    return eng.resample(torch.cat([torch.zeros(x.shape[0], z, device=DEV), x], dim=1), in_freq, out_freq)[:, :n_total]


def _signal(n, seed, scale=0.5):
    """[S, n] fp32, every stream its own content"""
    return (torch.randn(S, n, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _pcm(n, seed):
    """[S, n] int16 over the whole range, both ends included"""
    pcm = torch.randint(-32768, 32768, (S, n), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.int16)
    pcm[0, 0], pcm[1, -1] = -32768, 32767
    return pcm.to(DEV)


def _block_len(kind, in_freq, out_freq):
    orig, _ = _terms(in_freq, out_freq)
    return {"one_group": orig, "three_groups": 3 * orig, "block_1920": 1920 * in_freq // 24000}[kind]


# ---- the defining identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one_group", "three_groups", "block_1920"])
@pytest.mark.parametrize("in_freq,out_freq", PAIRS)
def test_blocks_equal_the_offline_resampler_with_zeros_in_front(in_freq, out_freq, kind):
    """7 blocks; `one_group` is shorter than the history for every pair (the state hand-over is part old state, part block)."""
    eng = _engine()
    n_in = _block_len(kind, in_freq, out_freq)
    n_out, hist, delay = eng.stream_resample_geometry(in_freq, out_freq, n_in)
    orig, new = _terms(in_freq, out_freq)
    assert n_out == n_in // orig * new and (kind != "one_group" or n_in < hist) and (kind != "block_1920" or 1920 in (n_in, n_out))
    x = _signal(N_BLOCKS * n_in, seed=in_freq // 100 + out_freq // 1000)
    state = torch.zeros(S, hist, device=DEV)
    history = torch.cat([torch.zeros(S, hist, device=DEV), x], dim=1)
    outs = []
    for b in range(N_BLOCKS):
        outs.append(eng.stream_resample(x[:, b * n_in:(b + 1) * n_in], state, in_freq, out_freq))
        assert outs[-1].shape == (S, n_out) and outs[-1].dtype == torch.float32
        assert _same(state, history[:, (b + 1) * n_in:(b + 1) * n_in + hist]), f"block {b}: the state is not the last {hist} samples of zeros ++ input"
    got = torch.cat(outs, dim=1)
    want = _offline(eng, x, in_freq, out_freq, n_in, N_BLOCKS * n_out)
    assert want.shape == got.shape and float(want.abs().max()) > 0      # (one group per block: 7 blocks are hardly past the delay)
    bad = (_bits(got) != _bits(want)).nonzero()
    assert _same(got, want), f"{in_freq} -> {out_freq}, n_in {n_in}: {len(bad)} samples differ from the offline result, first at (stream, sample) {bad[0].tolist()}"
    # and the definition holds for every prefix, not only the whole: the offline result of 3 blocks alone starts the same way
    assert _same(got[:, :3 * n_out], _offline(eng, x[:, :3 * n_in], in_freq, out_freq, n_in, 3 * n_out))
    assert not _same(got[0], got[1]) and not _same(got[1], got[2])


# ---- isolation ---------------------------------------------------------------------------------------------------------------------------
def _raw_call(eng, x, state_buf, out_buf, in_freq, out_freq):
    rc = eng.lib.tvc_stream_resample(eng.ctx, eng._stream(), ctypes.c_void_p(x.data_ptr()), 0, ctypes.c_void_p(out_buf.data_ptr()), 0,
                                     ctypes.c_void_p(state_buf.data_ptr()), S, x.shape[1], in_freq, out_freq, 0.0)
    assert rc == 0, eng.lib.tvc_last_error(eng.ctx)


@pytest.mark.parametrize("in_freq,out_freq,n_in", [(44100, 24000, 3 * 147), (48000, 24000, 3840), (24000, 44100, 80)])
def test_streams_do_not_see_each_other_and_nothing_is_written_past_the_rows(in_freq, out_freq, n_in):
    eng = _engine()
    n_out, hist, _ = eng.stream_resample_geometry(in_freq, out_freq, n_in)
    PAD = 64
    start = _signal(hist, seed=5)      # a history that is not zeros

    def run(x):
        state_buf = torch.full((S * hist + PAD,), POISON, device=DEV)
        state_buf[:S * hist] = start.reshape(-1)
        out_buf = torch.full((S * n_out + PAD,), POISON, device=DEV)
        _raw_call(eng, x, state_buf, out_buf, in_freq, out_freq)
        assert bool((state_buf[S * hist:] == POISON).all()) and bool((out_buf[S * n_out:] == POISON).all()), "written behind the last row"
        return out_buf[:S * n_out].view(S, n_out).clone(), state_buf[:S * hist].view(S, hist).clone()

    x = _signal(n_in, seed=6)
    out, state = run(x)
    assert not bool((out == POISON).any()) and not bool((state == POISON).any())
    other = x.clone()
    other[1] = _signal(n_in, seed=7)[1]
    out2, state2 = run(other)
    for s in (0, 2):
        assert _same(out[s], out2[s]) and _same(state[s], state2[s]), f"stream {s} changed when stream 1's input did"
    assert not _same(out[1], out2[1]) and not _same(state[1], state2[1])
    nan = x.clone()
    nan[1, 0] = float("nan")      # the block's first sample: inside the first output group's taps whatever the look-ahead
    out3, state3 = run(nan)
    assert bool(torch.isnan(out3[1]).any()), "the NaN did not reach its own stream's output"
    for s in (0, 2):
        assert _same(out[s], out3[s]) and _same(state[s], state3[s]), f"a NaN in stream 1 reached stream {s}"


# ---- the int16 forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain_db", [0.0, -6.0])
@pytest.mark.parametrize("in_freq,out_freq,n_in", [(44100, 24000, 147), (48000, 24000, 3840), (16000, 24000, 10), (8000, 24000, 643)])
def test_int16_in_equals_the_conversion_then_the_fp32_door(in_freq, out_freq, n_in, gain_db):
    """n_in = 147, 10 and 643 put the rows of the int16 block at every 2-byte offset of an 8-byte word (the 8-byte loads start at the first
    boundary inside the row); 3840 keeps them aligned."""
    eng = _engine()
    _, hist, _ = eng.stream_resample_geometry(in_freq, out_freq, n_in)
    s16, s32 = torch.zeros(S, hist, device=DEV), torch.zeros(S, hist, device=DEV)
    for b in range(3):
        pcm = _pcm(n_in, seed=10 + b)
        got = eng.stream_resample(pcm, s16, in_freq, out_freq, gain_db)
        want = eng.stream_resample(eng.pcm16_to_f32(pcm, gain_db), s32, in_freq, out_freq)
        assert _same(got, want) and _same(s16, s32), f"block {b}"
    assert float(got.abs().max()) > 0.1


@pytest.mark.parametrize("gain_db", [0.0, -6.0, 6.0])
@pytest.mark.parametrize("in_freq,out_freq,n_in", [(24000, 48000, 1920), (24000, 44100, 80), (24000, 8000, 99)])
def test_int16_out_equals_the_fp32_door_then_the_conversion(in_freq, out_freq, n_in, gain_db):
    """a signal several times full scale: the int16 values wrap as numpy's cast does, the same in both"""
    eng = _engine()
    _, hist, _ = eng.stream_resample_geometry(in_freq, out_freq, n_in)
    s16, s32 = torch.zeros(S, hist, device=DEV), torch.zeros(S, hist, device=DEV)
    wrapped = False
    for b in range(4):
        x = _signal(n_in, seed=20 + b, scale=4.0)
        got = eng.stream_resample(x, s16, in_freq, out_freq, gain_db, out_pcm16=True)
        mid = eng.stream_resample(x, s32, in_freq, out_freq)
        want = eng.f32_to_pcm16(mid, gain_db)
        assert got.dtype == torch.int16 and _same(got, want) and _same(s16, s32), f"block {b}"
        wrapped |= bool((mid.abs() * 10 ** (gain_db / 20) > 1.0).any())
    assert wrapped, "no value left the int16 range: the wrap-around was not exercised"


def test_equal_rates_run_the_plain_conversions():
    eng = _engine()
    assert eng.stream_resample_geometry(24000, 24000, 1000) == (1000, 0, 0)
    pcm, x = _pcm(1000, seed=30), _signal(1000, seed=31, scale=1.5)
    for gain_db in (0.0, -6.0):
        assert _same(eng.stream_resample(pcm, None, 24000, 24000, gain_db), eng.pcm16_to_f32(pcm, gain_db))
        assert _same(eng.stream_resample(x, None, 24000, 24000, gain_db, out_pcm16=True), eng.f32_to_pcm16(x, gain_db))
    y = eng.stream_resample(x, None, 24000, 24000)
    assert _same(y, x) and y.data_ptr() != x.data_ptr()


def test_the_library_refuses_what_the_header_says():
    from tinyvc_amd._lib import TinyVCError
    eng = _engine()
    x, pcm = _signal(3840, seed=1), _pcm(3840, seed=1)
    state = torch.zeros(S, 27, device=DEV)
    with pytest.raises(ValueError, match="whole 2-sample groups"):
        eng.stream_resample(x[:, :3839], state, 48000, 24000)
    with pytest.raises(ValueError, match=r"\[3, 27\]"):
        eng.stream_resample(x, torch.zeros(S, 26, device=DEV), 48000, 24000)
    with pytest.raises(TinyVCError, match="one side is fp32"):
        eng.stream_resample(pcm, state, 48000, 24000, out_pcm16=True)
    with pytest.raises(TinyVCError, match="gain_db belongs to the int16"):
        eng.stream_resample(x, state, 48000, 24000, gain_db=-6.0)
    assert not bool(state.any()), "a refused call touched the state"


# ---- StreamDoor ----------------------------------------------------------------------------------------------------------------------------
def test_door_geometry_and_reset():
    from tinyvc_amd.module.infer import StreamDoor
    eng = _engine()
    door = StreamDoor(S, 44100, 48000, block_size=1920, input_gain=-3.0, output_gain=2.0, device=DEV)
    assert (door.chunk_in, door.chunk_out, door.hist_in, door.hist_out, door.delay_in, door.delay_out) == (3528, 3840, 159, 14, 80, 14)
    assert door.latency_seconds == 80 / 24000 + 14 / 48000
    assert door.in_state.shape == (S, 159) and door.out_state.shape == (S, 14) and door.in_state.device == torch.device(DEV)
    door.prepare(eng)
    a, b = _pcm(3528, seed=40), _pcm(3528, seed=41)
    first = door.pull(eng, door.push(eng, a))
    assert first.shape == (S, 3840) and first.dtype == torch.int16
    second = door.pull(eng, door.push(eng, b))
    ptrs = (door.in_state.data_ptr(), door.out_state.data_ptr())
    door.reset()
    assert not bool(door.in_state.any()) and not bool(door.out_state.any()) and ptrs == (door.in_state.data_ptr(), door.out_state.data_ptr())
    again = door.pull(eng, door.push(eng, a))
    assert _same(again, first), "after reset() the stream does not start from the zero history"
    after_b = door.pull(eng, door.push(eng, b))
    assert _same(after_b, second)
    # one stream restarted, its neighbours carrying on
    door.reset([1])
    mixed = door.pull(eng, door.push(eng, a))
    assert _same(mixed[1], first[1]) and not _same(mixed[0], first[0]) and not _same(mixed[2], first[2])


# ---- a stream through a door == the chain of offline pieces ---------------------------------------------------------------------------------
E2E_BLOCKS = 6


@pytest.fixture(scope="module")
def gen():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    enc_sd, dec_sd = state_dicts(0)
    enc, dec = Encoder(), Decoder()
    enc.load_state_dict(enc_sd)
    dec.load_state_dict(dec_sd)
    return Generator(enc, dec).to(DEV)


@pytest.fixture(scope="module")
def model_side():
    tgt = synth.synth_index(1000, seed=2).to(DEV)
    angles = [synth.synth_angle(S, 28, 900 + i).to(DEV) for i in range(E2E_BLOCKS)]
    return tgt, angles


def _client_pcm(rate, n):
    """[S, n] int16 of speech-like synthetic audio at `rate`, every stream its own"""
    wf = synth.synth_wave(S, n, seed=60 + rate // 1000)
    return (wf * 0.8 * 32767).to(torch.int16).to(DEV)


def _door_stream(gen, tgt, door, use_graph=False):
    from tinyvc_amd.module.infer import BatchedStreamInfer
    st = BatchedStreamInfer(gen, n_streams=S, target=tgt, pitch_shift=[0.0, 2.0, -1.5], device=torch.device(DEV), block_size=1920, extra_size=3840,
                            use_graph=use_graph, door=door)
    st.init_buffer()
    return st


@pytest.mark.parametrize("in_rate,out_rate", [(48000, 48000), (44100, 48000)])
def test_a_stream_through_the_door_equals_the_offline_chain(gen, model_side, in_rate, out_rate):
    from tinyvc_amd.module.infer import StreamDoor
    tgt, angles = model_side
    eng = gen.engine(torch.device(DEV))
    door = StreamDoor(S, in_rate, out_rate, block_size=1920, input_gain=-3.0, output_gain=2.0, device=DEV)
    pcm = _client_pcm(in_rate, E2E_BLOCKS * door.chunk_in)
    st = _door_stream(gen, tgt, door)
    got = torch.cat([st.audio_callback_pcm(pcm[:, i * door.chunk_in:(i + 1) * door.chunk_in], noise_angle=angles[i]) for i in range(E2E_BLOCKS)], dim=1)
    assert got.dtype == torch.int16 and got.shape == (S, E2E_BLOCKS * door.chunk_out)
    # offline pieces only
    x24 = _offline(eng, eng.pcm16_to_f32(pcm, -3.0), in_rate, 24000, door.chunk_in, E2E_BLOCKS * 1920)
    plain = _door_stream(gen, tgt, None)
    y24 = torch.cat([plain.audio_callback(x24[:, i * 1920:(i + 1) * 1920], noise_angle=angles[i]) for i in range(E2E_BLOCKS)], dim=1)
    want = eng.f32_to_pcm16(_offline(eng, y24, 24000, out_rate, 1920, E2E_BLOCKS * door.chunk_out), 2.0)
    assert int(want.to(torch.int32).abs().max()) > 1000, "the chain is silent"
    bad = (got != want).nonzero()
    assert _same(got, want), f"{len(bad)} samples differ from the offline chain, first at (stream, sample) {bad[0].tolist()}"


def _run(gen, model_side, use_graph):
    from tinyvc_amd.module.infer import StreamDoor
    tgt, angles = model_side
    door = StreamDoor(S, 44100, 48000, block_size=1920, input_gain=-3.0, device=DEV)
    pcm = _client_pcm(44100, E2E_BLOCKS * door.chunk_in)
    st = _door_stream(gen, tgt, door, use_graph)
    outs, graphs = [], []
    for i in range(E2E_BLOCKS):
        if i == 4:
            door.reset()
        outs.append(st.audio_callback_pcm(pcm[:, i * door.chunk_in:(i + 1) * door.chunk_in], noise_angle=angles[i]).clone())
        graphs.append(st._graph[1][("pcm", True)][0] if use_graph and st._graph is not None and ("pcm", True) in st._graph[1] else None)
    return torch.stack(outs), (door.in_state.clone(), door.out_state.clone()), graphs, st


def test_graph_replay_equals_eager_with_one_capture(gen, model_side):
    """door.reset() before block 4 and the history advancing all along: the graph captured at block 2 replays to the end (the same graph
    object) and equals eager; another rate, block size or gain is another key."""
    from tinyvc_amd.module.infer import StreamDoor
    eager = _run(gen, model_side, False)
    graph = _run(gen, model_side, True)
    g = graph[2]
    assert g[0] is None and g[1] is None and g[2] is not None and all(x is g[2] for x in g[2:]), "a reset / the history advancing captured a new graph"
    assert _same(eager[0], graph[0]), "graph replay is not sample-exact"
    assert _same(eager[1][0], graph[1][0]) and _same(eager[1][1], graph[1][1]), "the final door state differs"
    assert not _same(eager[0][4], eager[0][3])
    # what re-captures
    st = graph[3]
    key = st._graph_key()
    assert key == st._graph[0]
    for kw in (dict(in_rate=48000), dict(out_rate=44100), dict(block_size=3840), dict(input_gain=0.0), dict(output_gain=1.0)):
        args = dict(in_rate=44100, out_rate=48000, block_size=1920, input_gain=-3.0, output_gain=0.0)
        args.update(kw)
        st.door = StreamDoor(S, device=DEV, **args)
        assert st._graph_key() != key, f"{kw} did not change the graph key"
    # a door at another rate on the same stream: the next block captures anew and comes out at the new rate
    st.door = StreamDoor(S, 44100, 44100, block_size=1920, input_gain=-3.0, device=DEV)
    st.door.prepare(gen.engine(torch.device(DEV)))
    out = st.audio_callback_pcm(_client_pcm(44100, 3528), noise_angle=model_side[1][0])
    assert out.shape == (S, 3528) and st._graph[1][("pcm", True)][0] is not g[2]


# ---- the entry script ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("door")
    torch.save(synth.synth_state_dict("encoder"), d / "encoder.pt")
    torch.save(synth.synth_state_dict("decoder"), d / "decoder.pt")
    torch.save(synth.synth_index(500, seed=2), d / "index.pt")
    audio_io.save(str(d / "mic.wav"), synth.synth_wave(3, E2E_BLOCKS * 1920, seed=50)[0:1] * 0.9, 24000)
    common = ["-encp", str(d / "encoder.pt"), "-decp", str(d / "decoder.pt"), "-idx", str(d / "index.pt"), "--input-wav", str(d / "mic.wav"), "--streams", "2",
              "-d", DEV, "-p", "0.5", "-ig", "-2", "-og", "1.5"]
    return d, common


def test_infer_streaming_resample_writes_what_the_class_loop_produces(files, capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamDoor
    d, common = files
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--resample", "-sr", "48000", "-c", "3840", "--output-wav", str(d / "door.wav")]) == 0
    text = capsys.readouterr().out
    assert "48000 Hz <-> 24000 Hz" in text and f"{(7 / 24000 + 14 / 48000) * 1e3:.2f} ms" in text and "p50" in text
    torch.manual_seed(3)
    dev = torch.device(DEV)
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), dev)
    door = StreamDoor(2, 48000, block_size=1920, input_gain=-2.0, output_gain=1.5, device=dev)
    st = BatchedStreamInfer(gen, n_streams=2, pitch_shift=0.5, block_size=1920, device=dev, extra_size=3840, door=door)
    st.target = torch.load(d / "index.pt").to(dev)
    st.init_buffer()
    outs = []
    for blk in infer_streaming.int16_blocks_from_wav(str(d / "mic.wav"), 48000, 3840, gen.engine(dev)):
        pcm = torch.from_numpy(np.ascontiguousarray(blk)).to(dev)
        outs.append(st.audio_callback_pcm(pcm.expand(2, -1)).cpu().numpy()[0])
    assert len(outs) == E2E_BLOCKS
    audio_io.save(str(d / "want.wav"), torch.from_numpy(np.concatenate(outs).astype(np.float32) / 32768)[None], 48000)
    assert open(d / "door.wav", "rb").read() == open(d / "want.wav", "rb").read()


def test_infer_streaming_resample_at_the_model_rate_changes_no_byte(files):
    import infer_streaming
    d, common = files
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--output-wav", str(d / "plain.wav")]) == 0
    torch.manual_seed(3)
    assert infer_streaming.main(common + ["--resample", "-sr", "24000", "-c", "1920", "--output-wav", str(d / "same.wav")]) == 0
    plain = open(d / "plain.wav", "rb").read()
    assert len(plain) > E2E_BLOCKS * 1920 * 2 and plain == open(d / "same.wav", "rb").read()
    # and both are the reference's loop body spelled out with the plain conversions around a door-less stream
    import infer
    from tinyvc_amd.module.infer import BatchedStreamInfer
    torch.manual_seed(3)
    dev = torch.device(DEV)
    gen = infer.load_generator(str(d / "encoder.pt"), str(d / "decoder.pt"), dev)
    st = BatchedStreamInfer(gen, n_streams=2, pitch_shift=0.5, block_size=1920, device=dev, extra_size=3840)
    st.target = torch.load(d / "index.pt").to(dev)
    st.init_buffer()
    eng = gen.engine(dev)
    outs = []
    for blk in infer_streaming.int16_blocks_from_wav(str(d / "mic.wav"), 24000, 1920, eng):
        x = eng.pcm16_to_f32(torch.from_numpy(np.ascontiguousarray(blk)).to(dev), -2.0)
        outs.append(eng.f32_to_pcm16(st.audio_callback(x.expand(2, -1)), 1.5).cpu().numpy()[0])
    audio_io.save(str(d / "loop.wav"), torch.from_numpy(np.concatenate(outs).astype(np.float32) / 32768)[None], 24000)
    assert plain == open(d / "loop.wav", "rb").read()
