"""The per-row alpha (tvc_knn_match_alpha_f32, tvc_convert_alpha_f32, tvc_convert_ragged_alpha_f32; Generator.convert(alpha=...)) without a GPU:
the new symbols are declared, bound and exported, alpha is normalised and refused on the host before any engine or device work, and the
entry scripts parse `--alpha` and leave their calls as they were when it is absent."""
import argparse

import pytest
import torch

from tinyvc_amd import _lib

NEW = ["tvc_knn_match_alpha_f32", "tvc_workspace_bytes_alpha", "tvc_convert_alpha_f32", "tvc_workspace_bytes_ragged_alpha", "tvc_convert_ragged_alpha_f32"]


@pytest.fixture(scope="module")
def lib():
    from tinyvc_amd import build
    build.build(verbose=False)
    return _lib.load_library()


def test_symbols_are_declared_bound_and_exported(lib):
    from test_cabi import header_functions
    decl = header_functions()
    for name in NEW:
        assert name in decl, f"{name} is not declared in tinyvc_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(decl[name]), name
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype is _lib.SIGNATURES[name][0], f"{name} is not bound with its signature"
    # each is its sibling's argument list plus `alpha`, behind `weights`
    for name, sibling in (("tvc_knn_match_alpha_f32", "tvc_knn_match_blend_f32"), ("tvc_convert_alpha_f32", "tvc_convert_track_f32"),
                          ("tvc_convert_ragged_alpha_f32", "tvc_convert_ragged_auto_f32")):
        args = [a.split()[-1].lstrip("*") for a in decl[name]]
        sib = [a.split()[-1].lstrip("*") for a in decl[sibling]]
        at = args.index("alpha")
        assert args[at - 1] == "weights" and args[:at] + args[at + 1:] == sib, name
        assert _lib.SIGNATURES[name][1][:at] + _lib.SIGNATURES[name][1][at + 1:] == _lib.SIGNATURES[sibling][1], name
    assert [a.split()[-1].lstrip("*") for a in decl["tvc_workspace_bytes_alpha"]] == [a.split()[-1].lstrip("*") for a in decl["tvc_workspace_bytes_auto"]]
    # argument checks come before any device work: no context, no call
    assert lib.tvc_workspace_bytes_alpha(None, 1, 4800, None, 1, None) == -1
    assert lib.tvc_workspace_bytes_ragged_alpha(None, 1, 4800, None, None, 1, None) == -1
    assert lib.tvc_knn_match_alpha_f32(None, None, None, None, None, 1, None, None, None, None, 1, 1, None, 0) == -1
    from tinyvc_amd import engine
    assert callable(engine.Engine.knn_match_alpha)
    assert engine._CONVERT["alpha", False] == ("tvc_workspace_bytes_alpha", "tvc_convert_alpha_f32")
    assert engine._CONVERT["alpha", True] == ("tvc_workspace_bytes_ragged_alpha", "tvc_convert_ragged_alpha_f32")
    assert engine._MATCH["alpha"] == ("tvc_workspace_bytes_alpha", "tvc_knn_match_alpha_f32")
    # the existing forms keep their entries
    assert engine._CONVERT["shared", False] == ("tvc_workspace_bytes", "tvc_convert_f32") and engine._MATCH["blend"][1] == "tvc_knn_match_blend_f32"
    assert engine._CONVERT["track", False][1] == "tvc_convert_track_f32" and len(engine._CONVERT) == 11 and len(engine._MATCH) == 4


def test_alpha_is_normalised_on_the_host():
    from tinyvc_amd.module.tinyvc.feature_retrieval import alpha_rows, resolve_alpha
    assert resolve_alpha(0.25, 3) == [0.25, 0.25, 0.25]
    assert resolve_alpha(1, 2) == [1.0, 1.0] and all(isinstance(x, float) for x in resolve_alpha(1, 2))
    assert resolve_alpha([0.0, 0.5, 1.5], 3) == [0.0, 0.5, 1.5]            # neither clamped nor normalised
    assert resolve_alpha((-0.25,), 3) == [-0.25] * 3                        # one entry: every row's
    assert resolve_alpha([0.3], 1) == [0.3]
    rows = alpha_rows(resolve_alpha([0.0, 0.5, 1.5], 3), 3, "cpu")
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.tolist() == [0.0, 0.5, 1.5]
    assert alpha_rows(resolve_alpha(0.75, 4), 4, "cpu").tolist() == [0.75] * 4
    for bad, why in (([0.1, 0.2], "2 shares for a batch of 3"), ([], "0 shares"), ("0.5", "alpha"), (None, "alpha"), (True, "alpha"), ([0.1, "x", 0.2], "alpha"),
                     (torch.zeros(3), "lives on the GPU"), (torch.zeros(2), "1 or B = 3"), (torch.zeros(3, 1), "1 or B = 3"),
                     (torch.zeros(3, dtype=torch.float64), "fp32"), (torch.zeros(3, dtype=torch.int32), "fp32")):
        with pytest.raises(ValueError, match=why):
            resolve_alpha(bad, 3)


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
        with pytest.raises(ValueError, match="alpha"):
            cpu_gen.convert(wf, plain, 0.0, alpha=bad)
    with pytest.raises(ValueError, match="alpha"):
        cpu_gen.convert(wf, [plain, plain], [0.0, 1.0], alpha=[0.5, 0.5, 0.5], lengths=[4800, 2400], auto_pitch=150.0)
    # a well-formed call gets as far as the device - and there is none; alpha=None never looks at alpha
    with pytest.raises(_lib.TinyVCError):
        cpu_gen.convert(wf, plain, 0.0, alpha=0.5)
    with pytest.raises(_lib.TinyVCError):
        cpu_gen.convert(wf, plain, 0.0, alpha=None)
    from tinyvc_amd.module.infer import BatchedStreamInfer
    with pytest.raises(ValueError, match="alpha"):
        BatchedStreamInfer(cpu_gen, n_streams=2, alpha=[0.1, 0.2, 0.3], device="cuda")
    st = BatchedStreamInfer(cpu_gen, n_streams=2, device="cuda")
    assert st.alpha is None


def test_entry_scripts_parse_alpha_and_leave_the_call_alone_without_it(capsys):
    import infer
    import infer_streaming
    from tinyvc_amd.module.tinyvc.feature_retrieval import alpha_keywords
    for mod, name in ((infer, "infer.py"), (infer_streaming, "infer_streaming.py")):
        absent = mod.build_parser().parse_args([])
        assert absent.alpha is None
        assert alpha_keywords(absent, name) == {} and capsys.readouterr().out == ""      # nothing added to the call, nothing printed
        given = mod.build_parser().parse_args(["--alpha", "0.25"])
        assert given.alpha == 0.25
        assert alpha_keywords(given, name) == {"alpha": 0.25}
        out = capsys.readouterr().out
        assert out.count("\n") == 1 and "0.25" in out and "alpha" in out                   # one line when it is set
        assert mod.build_parser().parse_args(["--alpha", "-0.5"]).alpha == -0.5              # extrapolation is legal
        with pytest.raises(SystemExit):
            alpha_keywords(argparse.Namespace(alpha=float("nan")), name)
    # the keyword reaches the conversions: infer.py's chunked path hands it to the streams
    import inspect
    assert "stream_kw" in inspect.signature(infer.convert_chunked).parameters
    assert "alpha" in inspect.signature(infer_streaming.BatchedStreamInfer.__init__).parameters
