"""protect - a per-frame share of the source from the call's own f0 (tvc_convert_protect_f32, tvc_convert_ragged_protect_f32,
tvc_knn_match_protect_f32, tvc_frame_share_f32; Generator.convert(protect=), BatchedStreamInfer(protect=)) - without a GPU: the new symbols
are declared, bound and exported, the engine's tables carry them, protect is normalised and refused on the host under its own name before
any engine or device work, and the entry scripts parse `--protect` and leave their calls alone when it is absent.

The pure-torch restatement of the definition lives here (frame_weights, frame_share, protect_bound, alpha_bound): tests/test_gpu_protect.py
imports it and holds the kernels to it bit for bit."""
import argparse

import pytest
import torch

from tinyvc_amd import _lib

NEW = ["tvc_workspace_bytes_protect", "tvc_convert_protect_f32", "tvc_workspace_bytes_ragged_protect", "tvc_convert_ragged_protect_f32",
       "tvc_knn_match_protect_f32", "tvc_frame_share_f32"]


# ---- the definition (include/tinyvc_hip.h), restated in eager torch on fp32 tensors: every operation rounds on its own ----
def frame_weights(f0):
    """f0 [T] of ONE utterance -> w [T] fp32 = 1 - (u[t-1] + 2 u[t] + u[t+1]) / 4, u = f0 > 0 (NaN, negatives: 0), u[-1] = u[0], u[T] = u[T-1]"""
    u = (f0 > 0).to(torch.float32)
    pad = torch.cat([u[:1], u, u[-1:]])
    return 1 - (pad[:-2] + 2 * u + pad[2:]) / 4


def frame_share(f0, a, p):
    """a_t [T] fp32 of one utterance: a + (1 - a) * (p * w); a, p floats (made fp32) or 0-dim fp32 tensors"""
    a = torch.as_tensor(a, dtype=torch.float32, device=f0.device)
    p = torch.as_tensor(p, dtype=torch.float32, device=f0.device)
    return a + (1 - a) * (p * frame_weights(f0))


def alpha_bound(a, idx_bound, srcmax):
    """the alpha call's content bound (fp32 tensors of equal shape)"""
    return (1 - a).abs() * idx_bound + a.abs() * srcmax


def protect_bound(a, p, idx_bound, srcmax):
    """the protect call's: every a_t lies between a and a_u = a + (1 - a) * p"""
    au = a + (1 - a) * p
    return torch.maximum((1 - a).abs(), (1 - au).abs()) * idx_bound + torch.maximum(a.abs(), au.abs()) * srcmax


def test_the_restatement_has_the_definitions_properties():
    f0 = torch.tensor([0.0, 0.0, 120.0, 130.0, 0.0, 140.0, float("nan"), -5.0, 20.0, 200.0, 210.0, 0.0])
    w = frame_weights(f0)
    #                    u = 0 0 1 1 0 1 0 0 1 1 1 0; the edges repeat themselves
    assert w.tolist() == [1.0, 0.75, 0.25, 0.25, 0.5, 0.5, 0.75, 0.75, 0.25, 0.0, 0.25, 0.75]
    assert frame_weights(torch.tensor([150.0])).tolist() == [0.0] and frame_weights(torch.tensor([0.0])).tolist() == [1.0]
    assert set(w.tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    for a in (0.0, 0.35, 1.5, -0.25):
        a32 = torch.tensor(a, dtype=torch.float32)
        assert torch.equal(frame_share(f0, a, 0.0), a32.expand(12)), "p = 0 must give a_t == a"
        at = frame_share(f0, a, 0.5)
        assert torch.equal(at[w == 0], a32.expand(int((w == 0).sum()))), "a fully voiced neighbourhood is untouched by p"
        lo, hi = sorted((float(a32), float(a32 + (1 - a32) * 0.5)))
        assert float(at.min()) >= lo and float(at.max()) <= hi, "every a_t lies between a and a_u"
    assert frame_share(f0, 0.0, 1.0)[0] == 1.0      # a = 0, p = 1, w = 1: the source's own bits (mu * 0 + src * 1)
    # the composition of index rate and protect on a fully unvoiced frame: the match keeps (1 - a)(1 - p)
    assert abs(1 - float(frame_share(torch.zeros(3), 0.25, 0.5)[1]) - (1 - 0.25) * (1 - 0.5)) < 1e-7
    g = torch.Generator().manual_seed(1)
    a = torch.tensor([0.0, 0.35, 1.5, -0.25, 1.0])
    ib, sm = torch.rand(5, generator=g) * 3, torch.rand(5, generator=g) * 40
    assert torch.equal(protect_bound(a, torch.zeros(5), ib, sm), alpha_bound(a, ib, sm)), "the bound at p = 0 is alpha's"
    assert torch.equal(protect_bound(torch.zeros(5), torch.zeros(5), ib, sm), ib), "... and at a = 0 too the index's own"
    p = torch.tensor([0.5, 1.0, 0.25, 0.75, 0.3])
    assert (protect_bound(a, p, ib, sm) >= alpha_bound(a, ib, sm)).all()


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def _names(decl, name):
    return [a.split()[-1].lstrip("*") for a in decl[name]]


def test_symbols_are_declared_bound_and_exported(lib):
    from test_cabi import header_functions
    decl = header_functions()
    for name in NEW:
        assert name in decl, f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl[name]), name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0], f"{name} is not bound with its signature"
    # each conversion is its alpha sibling's argument list plus `protect`, behind `alpha`
    for name, sibling in (("tvc_convert_protect_f32", "tvc_convert_alpha_f32"), ("tvc_convert_ragged_protect_f32", "tvc_convert_ragged_alpha_f32")):
        args, sib = _names(decl, name), _names(decl, sibling)
        at = args.index("protect")
        assert args[at - 1] == "alpha" and args[:at] + args[at + 1:] == sib, name
        assert _lib.SIGNATURES[name][1][:at] + _lib.SIGNATURES[name][1][at + 1:] == _lib.SIGNATURES[sibling][1], name
    # the stage call: the alpha stage call plus f0 behind src and protect behind alpha
    args = _names(decl, "tvc_knn_match_protect_f32")
    assert args[args.index("f0") - 1] == "src" and args[args.index("protect") - 1] == "alpha"
    assert [a for a in args if a not in ("f0", "protect")] == _names(decl, "tvc_knn_match_alpha_f32")
    for q, sib in (("tvc_workspace_bytes_protect", "tvc_workspace_bytes_alpha"), ("tvc_workspace_bytes_ragged_protect", "tvc_workspace_bytes_ragged_alpha")):
        assert _names(decl, q) == _names(decl, sib) and _lib.SIGNATURES[q] == _lib.SIGNATURES[sib]
    assert _names(decl, "tvc_frame_share_f32") == ["ctx", "stream", "f0", "row_start", "row_count", "rows", "alpha", "protect", "share_out"]
    # argument checks come before any device work: no context, no call
    assert lib.tvc_workspace_bytes_protect(None, 1, 4800, None, 1, None) == -1
    assert lib.tvc_workspace_bytes_ragged_protect(None, 1, 4800, None, None, 1, None) == -1
    assert lib.tvc_knn_match_protect_f32(None, None, None, None, None, None, 1, None, None, None, None, None, 1, 1, None, 0) == -1
    assert lib.tvc_frame_share_f32(None, None, None, None, None, 1, None, None, None) == -1


def test_the_engine_tables_carry_the_entries():
    from tinyvc_amd import engine
    assert engine._PROTECT == {False: ("tvc_workspace_bytes_protect", "tvc_convert_protect_f32"),
                               True: ("tvc_workspace_bytes_ragged_protect", "tvc_convert_ragged_protect_f32"),
                               "match": ("tvc_workspace_bytes_protect", "tvc_knn_match_protect_f32")}
    assert engine._names("protect", False)[1] == "tvc_convert_protect_f32" and engine._names("protect", True)[1] == "tvc_convert_ragged_protect_f32"
    assert engine._names("protect") == ("tvc_workspace_bytes_protect", "tvc_knn_match_protect_f32")
    # one lookup for every form: the existing rows are found through it, unchanged
    for (form, ragged), names in engine._CONVERT.items():
        assert engine._names(form, ragged) == names
    for form, names in engine._MATCH.items():
        assert engine._names(form) == names
    assert engine._CONVERT["alpha", False][1] == "tvc_convert_alpha_f32" and engine._MATCH["alpha"][1] == "tvc_knn_match_alpha_f32"
    for name in ("knn_match_protect", "frame_share"):
        assert callable(getattr(engine.Engine, name))
    import inspect
    assert "protect" in inspect.signature(engine.Engine._convert).parameters


def test_protect_is_normalised_on_the_host_by_alphas_code():
    from tinyvc_amd.module.tinyvc.feature_retrieval import protect_rows, resolve_alpha, resolve_protect
    assert resolve_protect(0.25, 3) == [0.25, 0.25, 0.25]
    assert resolve_protect(1, 2) == [1.0, 1.0] and all(isinstance(x, float) for x in resolve_protect(1, 2))
    assert resolve_protect([0.0, 0.5, 1.5], 3) == [0.0, 0.5, 1.5]            # neither clamped nor normalised
    assert resolve_protect((-0.25,), 3) == [-0.25] * 3
    rows = protect_rows(resolve_protect([0.0, 0.5, 1.0], 3), 3, "cpu")
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.tolist() == [0.0, 0.5, 1.0]
    for bad, why in (([0.1, 0.2], "2 shares for a batch of 3"), ([], "0 shares"), ("0.5", "protect"), (None, "protect"), (True, "protect"),
                     ([0.1, "x", 0.2], "protect"), (torch.zeros(3), "lives on the GPU"), (torch.zeros(2), "1 or B = 3"), (torch.zeros(3, 1), "1 or B = 3"),
                     (torch.zeros(3, dtype=torch.float64), "fp32"), (torch.zeros(3, dtype=torch.int32), "fp32")):
        with pytest.raises(ValueError, match=why) as e:
            resolve_protect(bad, 3)
        assert str(e.value).startswith("protect:") and "alpha" not in str(e.value)
    # one resolver under two names: alpha's own messages are what they were
    with pytest.raises(ValueError, match="^alpha: 2 shares for a batch of 3"):
        resolve_alpha([0.1, 0.2], 3)


@pytest.fixture(scope="module")
def cpu_gen():
    """a Generator that never left the CPU: whatever reaches its engine raises TinyVCError (a RuntimeError), never ValueError"""
    from tinyvc_amd.module.infer import Generator
    from tinyvc_amd.module.tinyvc import Decoder, Encoder
    return Generator(Encoder(), Decoder())


def test_refusals_come_before_device_work(cpu_gen):
    wf = torch.zeros(2, 4800)
    plain = torch.zeros(1, 768, 8)
    for bad in ([0.1, 0.2, 0.3], "0.5", True, torch.zeros(2), torch.zeros(3), torch.zeros(2, dtype=torch.float16)):
        with pytest.raises(ValueError, match="protect"):
            cpu_gen.convert(wf, plain, 0.0, protect=bad)
        with pytest.raises(ValueError, match="protect"):
            cpu_gen.convert(wf, plain, 0.0, alpha=0.5, protect=bad)
    with pytest.raises(ValueError, match="protect"):
        cpu_gen.convert(wf, [plain, plain], [0.0, 1.0], alpha=[0.5, 0.5], protect=[0.5, 0.5, 0.5], lengths=[4800, 2400], auto_pitch=150.0)
    # a well-formed call gets as far as the device - and there is none; protect=None never looks at protect
    for kw in ({"protect": 0.5}, {"protect": [0.5, 1.0], "alpha": 0.25}, {"protect": None}):
        with pytest.raises(_lib.TinyVCError):
            cpu_gen.convert(wf, plain, 0.0, **kw)
    from tinyvc_amd.module.infer import BatchedStreamInfer, StreamInfer
    with pytest.raises(ValueError, match="protect"):
        BatchedStreamInfer(cpu_gen, n_streams=2, protect=[0.1, 0.2, 0.3], device="cuda")
    with pytest.raises(ValueError, match="protect"):
        StreamInfer(cpu_gen, protect="1")
    st = BatchedStreamInfer(cpu_gen, n_streams=2, device="cuda")
    assert st.protect is None and st.alpha is None


def test_entry_scripts_parse_protect_and_leave_the_call_alone_without_it(capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.tinyvc.feature_retrieval import alpha_keywords
    for mod, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        absent = mod.build_parser().parse_args([])
        assert absent.protect is None
        assert alpha_keywords(absent, name) == {} and capsys.readouterr().out == ""      # nothing added to the call, nothing printed
        given = mod.build_parser().parse_args(["--protect", "0.5"])
        assert given.protect == 0.5 and given.alpha is None
        assert alpha_keywords(given, name) == {"protect": 0.5}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "0.5" in out and "protect" in out
        both = mod.build_parser().parse_args(["--alpha", "0.25", "--protect", "1"])
        assert alpha_keywords(both, name) == {"alpha": 0.25, "protect": 1.0}
        assert capsys.readouterr().out.count("\n") == 2
        with pytest.raises(SystemExit):
            alpha_keywords(argparse.Namespace(alpha=None, protect=float("inf")), name)
    import inspect
    from tinyvc_amd.module.infer import Generator, StreamInfer
    assert "protect" in inspect.signature(infer_streaming.BatchedStreamInfer.__init__).parameters
    assert "protect" in inspect.signature(StreamInfer.__init__).parameters and "protect" in inspect.signature(Generator.convert).parameters
