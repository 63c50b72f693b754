"""Which C entry every form of Generator.convert reaches, pinned.

target                  pitch_shift   auto_pitch   query / entry (equal; ragged: tvc_workspace_bytes_ragged* / tvc_convert_ragged*_f32)
shared [1, 768, N]      scalar        off          tvc_workspace_bytes        / tvc_convert_f32
shared                  per row       off          tvc_workspace_bytes_multi  / tvc_convert_multi_f32, the shared blob in every row
table (tensor or list)  any           off          tvc_workspace_bytes_multi  / tvc_convert_multi_f32
Blend                   any           off          tvc_workspace_bytes_blend  / tvc_convert_blend_f32
shared or table         any           on           tvc_workspace_bytes_auto   / tvc_convert_auto_f32, no weights (shared: the blob in every row)
Blend                   any           Hz           tvc_workspace_bytes_auto   / tvc_convert_auto_f32 with the blend's weights

Every call makes exactly one workspace query and one conversion, and its waveform is the one the matching public Engine method returns for
the resolved blobs.  A call refused for its shift list leaves torch's generator where it was."""
import pytest
import torch

from helpers import state_dicts
from tinyvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L = 2, 9600                      # 20 frames
LENGTHS = [9600, 6000]              # 20 and 13 frames: one length class, one in-kernel batch
HZ = 150.0


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
def inputs():
    from tinyvc_amd.module.tinyvc import Blend
    wf = synth.synth_wave(B, L, seed=91)
    wf[1, LENGTHS[1]:] = 0
    a, b = synth.synth_index(64, seed=92).to(DEV), synth.synth_index(300, seed=93).to(DEV)
    return {"wf": wf.to(DEV), "angle": synth.synth_angle(B, L // 480, 94).to(DEV), "a": a, "b": b,
            "stacked": torch.cat([synth.synth_index(64, seed=95), synth.synth_index(64, seed=96)]).to(DEV),
            "blend": Blend([a, b], [0.7, 0.3])}


class LibSpy:
    """forwards everything to the library; records the name of every tvc_convert* / tvc_workspace_bytes* function called"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("tvc_convert", "tvc_workspace_bytes")):
            return fn

        def recorded(*args):
            self.names.append(name)
            return fn(*args)
        return recorded


def spied(eng, call):
    spy = LibSpy(eng.lib)
    eng.lib = spy
    try:
        out = call()
    finally:
        eng.lib = spy._lib
    return out, spy.names


def _prepared(tgt):
    """the (blobs, Ns, weights) tables the engine takes for a target of B rows"""
    from tinyvc_amd.module.tinyvc import Blend
    from tinyvc_amd.module.tinyvc.feature_retrieval import prepare_reference, prepare_references
    if isinstance(tgt, Blend):
        return tgt.resolve(B, torch.device(DEV))
    if isinstance(tgt, torch.Tensor) and tgt.shape[0] == 1:
        blob, n = prepare_reference(tgt)
        return [blob] * B, [n] * B, None
    return (*prepare_references(tgt), None)


# name: (target, pitch_shift, auto_pitch, family of C names, the public Engine methods (equal, ragged))
ROUTES = {
    "shared, scalar": ("a", 1.0, None, "", ("convert", "convert_ragged")),
    "shared, a shift per row": ("a", [1.0, -2.0], None, "_multi", ("convert_multi", "convert_ragged_multi")),
    "list, scalar": (("a", "b"), 1.0, None, "_multi", ("convert_multi", "convert_ragged_multi")),
    "tensor of B rows, a shift per row": ("stacked", [1.0, -2.0], None, "_multi", ("convert_multi", "convert_ragged_multi")),
    "blend, scalar": ("blend", 1.0, None, "_blend", ("convert_blend", "convert_ragged_blend")),
    "blend, a shift per row": ("blend", [1.0, -2.0], None, "_blend", ("convert_blend", "convert_ragged_blend")),
    "shared, auto, scalar": ("a", 1.0, HZ, "_auto", ("convert_auto", "convert_ragged_auto")),
    "shared, auto, a shift per row": ("a", [1.0, -2.0], HZ, "_auto", ("convert_auto", "convert_ragged_auto")),
    "list, auto": (("a", "b"), 1.0, HZ, "_auto", ("convert_auto", "convert_ragged_auto")),
    "blend, auto in Hz": ("blend", 1.0, HZ, "_auto", ("convert_auto", "convert_ragged_auto")),
}


@pytest.mark.parametrize("ragged", [False, True], ids=["equal", "ragged"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route(gen, inputs, route, ragged):
    key, shift, auto, family, methods = ROUTES[route]
    tgt = [inputs[k] for k in key] if isinstance(key, tuple) else inputs[key]
    wf, angle = inputs["wf"], inputs["angle"]
    lengths = LENGTHS if ragged else None
    eng = gen.engine(torch.device(DEV))
    res, names = spied(eng, lambda: gen.convert(wf, tgt, shift, noise_angle=angle, lengths=lengths, auto_pitch=auto, return_shift=auto is not None))
    r = "_ragged" if ragged else ""
    assert names == [f"tvc_workspace_bytes{r}{family}", f"tvc_convert{r}{family}_f32"], f"{route}: the call reached {names}"

    # the same call through the public Engine method, with the blobs resolved here
    method = getattr(eng, methods[ragged])
    lens = ([-(-n // 480) * 480 for n in LENGTHS],) if ragged else ()      # in whole frames, as the engine takes them
    blobs, ns, w = _prepared(tgt)
    if family == "":
        want = method(wf, *lens, blobs[0], ns[0], shift, angle)
    elif family == "_multi":
        want = method(wf, *lens, blobs, ns, shift, angle)
    elif family == "_blend":
        want = method(wf, *lens, blobs, ns, w, shift, angle)
    else:
        want = method(wf, *lens, blobs, ns, torch.full((B,), HZ, device=DEV), shift, w, angle)
        assert torch.equal(res[1], want[1]), f"{route}: the shifts differ from Engine.{methods[ragged]}'s"
        res, want = res[0], want[0]
    assert res.shape == (B, L) and torch.equal(res, want), f"{route}: the waveform differs from Engine.{methods[ragged]}'s"
    if ragged:
        assert not res[1, 6240:].any()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_refused_shift_list_draws_nothing(gen, inputs, route):
    """noise_angle=None makes the engine read and advance torch's generator for the library's seed - only once the call has passed every
    host check"""
    key, _shift, auto, _family, _methods = ROUTES[route]
    tgt = [inputs[k] for k in key] if isinstance(key, tuple) else inputs[key]
    g = torch.cuda.default_generators[0]
    eng = gen.engine(torch.device(DEV))
    off = g.get_offset()
    for lengths in (None, LENGTHS):
        with pytest.raises(ValueError, match="3 shifts for a batch of 2"):
            gen.convert(inputs["wf"], tgt, [1.0, 2.0, 3.0], lengths=lengths, auto_pitch=auto)
    assert g.get_offset() == off, "a refused call advanced the generator"
    blobs, ns, _w = _prepared(inputs["a"])
    with pytest.raises(ValueError):
        eng.convert_multi(inputs["wf"], blobs, ns, [1.0, 2.0, 3.0])
    assert g.get_offset() == off, "a call the engine refused advanced the generator"
