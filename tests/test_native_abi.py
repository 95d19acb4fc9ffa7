"""CPU: the C-ABI library builds for gfx950 here, loads, and exports every symbol include/captioner_hip.h declares.
No compute call is made (no GPU in this container)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "captioner_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cap_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_surface():
    names = _declared()
    for must in ("cap_create", "cap_destroy", "cap_load_weight", "cap_finalize_weights", "cap_encode", "cap_generate",
                 "cap_last_error"):
        assert must in names


def test_library_builds_loads_and_exports_all_symbols():
    from embodied_captioning_amd import _native, build
    path = build.build(verbose=False)
    assert os.path.exists(path)
    lib = _native.load_library()
    for name in _declared():
        assert hasattr(lib, name), f"{name} declared in include/captioner_hip.h but not exported"
    assert set(_native.EXPORTS) == set(_declared())
    assert lib.cap_version() >= 1
    assert lib.cap_last_error() is not None


def test_config_struct_matches_header_field_order():
    from embodied_captioning_amd import _native
    text = open(os.path.join(ROOT, "include", "captioner_hip.h")).read()
    body = re.search(r"typedef struct CapConfig \{(.*?)\} CapConfig;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        _, names = decl.split(None, 1)
        for n in names.split(","):
            fields.append(re.sub(r"\[.*\]", "", n).strip())
    assert fields == [f[0] for f in _native.CapConfig._fields_]


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from embodied_captioning_amd._native import CaptionerHipError
    from embodied_captioning_amd.config import BlipArch
    from embodied_captioning_amd.engine import CaptionerEngine
    with pytest.raises(CaptionerHipError):
        CaptionerEngine(BlipArch.tiny())


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "embodied_captioning_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith(".py"):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, fn)


def test_arena_debug_calls_are_bound_by_the_engine_module_alone():
    """cap_debug_fill_arena / cap_debug_arena_kinds are for tests/test_arena_state_gpu.py: bound in _native.py, wrapped once in
    engine.py (`_fill_arena`, `_arena_kinds`), named by no other module of the product package."""
    pkg = os.path.join(ROOT, "embodied_captioning_amd")
    users = set()
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith(".py") and re.search(r"cap_debug_|_fill_arena|_arena_kinds", open(os.path.join(dp, fn)).read()):
                users.add(os.path.relpath(os.path.join(dp, fn), pkg))
    assert users == {"_native.py", "engine.py"}


@pytest.mark.skipif(os.environ.get("CAP_RUN_ASAN") != "1", reason="rebuilds every .hip file with -fsanitize=address (~2 min): "
                    "set CAP_RUN_ASAN=1; the committed run is profiles/r02_asan_host.txt")
def test_host_side_asan_run_of_the_abi_argument_handling(tmp_path):
    """SURVEY.md section 5 (sanitizers): the host half of the library under AddressSanitizer + LeakSanitizer - every failing
    cap_create / cap_load_weight / launcher argument check returns an error code with nothing leaked or overrun."""
    import subprocess
    log = tmp_path / "asan.log"
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_host_check.sh"), str(log)], capture_output=True, text=True)
    text = log.read_text() if log.exists() else ""
    assert r.returncode == 0 and "0 failures" in text and "ERROR: AddressSanitizer" not in text, r.stderr + text
