"""The native C ABI is declared once, in ``madnn/ops/csrc/abi.h``: every C-linkage ``madnn_*`` function a ``.hip``
file defines has exactly one declaration there, no other file carries a hand copy, and the compiler rejects a
definition that disagrees with it (source scans and one syntax-only compile; no GPU, no built library)."""
import re
import subprocess

import pytest

from madnn import ops
from madnn.ops import build

_TYPE = r"(?:const )?(?:unsigned )?\w+\*?"
# at column 0 (function bodies are indented): a return type, the name, the parameter list, then a body or a ';'
_DEF = re.compile(rf'^(?:extern "C" )?{_TYPE} (madnn_\w+)\([^)]*\)\s*\{{', re.M)
_DECL = re.compile(rf'^(?:extern "C" )?{_TYPE} (madnn_\w+)\([^)]*\)\s*;', re.M)


def _code(name):
    return re.sub(r"//[^\n]*", "", (build.CSRC / name).read_text())


def test_every_entry_point_is_declared_once():
    defined = [n for s in build.KERNEL_SOURCES if s.endswith(".hip") for n in _DEF.findall(_code(s))]
    declared = _DECL.findall(_code("abi.h"))
    assert len(defined) > 100 and len(set(defined)) == len(defined)
    assert sorted(declared) == sorted(set(declared)), "a name is declared twice in abi.h"
    assert set(declared) == set(defined), sorted(set(declared) ^ set(defined))


def test_no_stray_prototypes():
    for f in sorted(build.CSRC.iterdir()):
        if f.name not in ("abi.h", "attn.h"):
            assert _DECL.findall(_code(f.name)) == [], f.name
    for s in build.KERNEL_SOURCES:
        if re.search(r"\bmadnn_\w+\(", _code(s)):
            assert '#include "abi.h"' in _code(s), s


_UNIT = """#include "abi.h"
extern "C" hipError_t madnn_conv1x1_fwd(const void* x, const void* w, void* y, float* stats, %s M, int64_t cin,
                                        int64_t cout, hipStream_t s) {
  return hipSuccess;
}
"""


def test_mismatched_definition_does_not_compile(tmp_path):
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        pytest.skip("no hipcc")
    res = {}
    for m_type in ("int64_t", "int"):
        src = tmp_path / f"unit_{m_type}.hip"
        src.write_text(_UNIT % m_type)
        res[m_type] = subprocess.run([hipcc, *build._flags_kernels(), "--offload-host-only", "-fsyntax-only", str(src)],
                                     capture_output=True, text=True)
    assert res["int64_t"].returncode == 0, res["int64_t"].stderr
    assert res["int"].returncode != 0 and "conflicting types" in res["int"].stderr, res["int"].stderr


def test_native_tune_unknown_family():
    if not ops.native_available():
        pytest.skip("kernel library not built")
    with pytest.raises(ValueError, match="nosuch"):
        ops.native_tune("nosuch", 0)
