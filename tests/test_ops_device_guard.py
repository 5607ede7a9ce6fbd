"""CPU check of the promise in the docstring of rstnet_amd/ops.py: every public function that takes the current stream runs under
the device guard of its first tensor argument (``@_on_tensor_device`` on the definition), so that a process may drive ``cuda:N``
without making it the current device.  No library and no GPU are needed: the functions are inspected, not called."""
import types

from rstnet_amd import ops

# launchers that enter `torch.cuda.device(...)` themselves instead of being wrapped
OWN_GUARD = {
    "rope_table": "takes the device as an argument (no tensor to read it from) and launches inside `with torch.cuda.device(device)`",
    "flush_hist_updates": "takes a list of (x, hist) pairs and launches inside `with torch.cuda.device(...)` of the first pair",
}


def _names(code: types.CodeType) -> set:
    """Global names `code`, or a function / lambda / comprehension nested in it, refers to."""
    names = set(code.co_names)
    for c in code.co_consts:
        if isinstance(c, types.CodeType):
            names |= _names(c)
    return names


def _uses_stream(code: types.CodeType, seen=None) -> bool:
    """`code` refers to `_stream`, itself or through the private helpers of the module it calls (`_gemm`, `_scratch`, ...)."""
    seen = set() if seen is None else seen
    for name in _names(code) - seen:
        seen.add(name)
        helper = vars(ops).get(name)
        if name == "_stream" or (name.startswith("_") and isinstance(helper, types.FunctionType) and _uses_stream(helper.__code__, seen)):
            return True
    return False


def _guard_code() -> types.CodeType:
    return ops._on_tensor_device(lambda: None).__code__


def public_launchers():
    out = {}
    for name, fn in vars(ops).items():
        if name.startswith("_") or not isinstance(fn, types.FunctionType) or fn.__module__ != ops.__name__:
            continue
        inner = getattr(fn, "__wrapped__", fn)
        if _uses_stream(inner.__code__):
            out[name] = fn
    return out


def test_scan_finds_the_launchers():
    found = public_launchers()
    assert len(found) >= 40, sorted(found)
    for name in ("gemm_win", "linear", "attention_step", "attention_qkv", "quantize_rows_fp8", "gemv_fp8w", "rope_table"):
        assert name in found, name


def test_every_public_launcher_runs_under_the_device_guard():
    guard = _guard_code()
    unguarded = sorted(name for name, fn in public_launchers().items() if fn.__code__ is not guard and name not in OWN_GUARD)
    assert unguarded == [], f"public launchers of rstnet_amd.ops without @_on_tensor_device: {unguarded}"


def test_self_guarding_launchers_enter_the_device_themselves():
    for name in OWN_GUARD:
        fn = getattr(ops, name)
        assert fn.__code__ is not _guard_code(), f"{name} is wrapped now: drop it from OWN_GUARD"
        assert "device" in fn.__code__.co_names and "cuda" in fn.__code__.co_names, name
