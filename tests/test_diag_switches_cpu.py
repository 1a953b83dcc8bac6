"""The kernels' wrong-result timing switches (KVEDGE_PP_ABL, KVEDGE_DIRECT_DIAG,
KVEDGE_C2F_DIAG, KVEDGE_NMS_DIAG) are compile-time macros of variant builds
(KVEDGE_VARIANT + KVEDGE_CFLAGS): nothing in the default library reads them from the
environment, and the default build defines none of them.  Runs on the CPU."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("KVEDGE_PP_ABL", "KVEDGE_DIRECT_DIAG", "KVEDGE_C2F_DIAG", "KVEDGE_NMS_DIAG")


def test_no_getenv_of_a_diag_switch_in_csrc():
    srcs = [p for p in glob.glob(os.path.join(ROOT, "csrc", "**", "*"), recursive=True)
            if os.path.isfile(p)]
    assert srcs
    hits = []
    for p in srcs:
        with open(p, errors="replace") as f:
            for name in re.findall(r'getenv\s*\(\s*"([^"]*)"', f.read()):
                if name.endswith("_DIAG") or name == "KVEDGE_PP_ABL":
                    hits.append((os.path.relpath(p, ROOT), name))
    assert not hits, hits


def test_default_build_defines_no_diag_switch(monkeypatch):
    for v in ("KVEDGE_VARIANT", "KVEDGE_CFLAGS", "KVEDGE_CHECKS"):
        monkeypatch.delenv(v, raising=False)
    # a private copy of the module: its flags are fixed from the environment at import
    spec = importlib.util.spec_from_file_location(
        "_kvedge_build_default", os.path.join(ROOT, "kvedge_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SO_PATH.endswith(os.path.join("kvedge_amd", "_C.so"))
    assert not [f for f in mod.COMMON if any(s in f for s in SWITCHES)], mod.COMMON


def test_default_library_does_not_name_the_switches():
    so = os.path.join(ROOT, "kvedge_amd", "_C.so")
    if not os.path.exists(so):
        pytest.skip("native library not built")
    with open(so, "rb") as f:
        blob = f.read()
    assert not [s for s in SWITCHES if s.encode() in blob]
