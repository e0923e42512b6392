"""CPU-only: the multi-view entries are declared in include/mi_depth.h, exported by the library and mirrored in the Python layer."""
import os
import re

from burn_depth_amd import _lib, ops
from burn_depth_amd.depth_anything3 import DepthAnything3
from burn_depth_amd.pipeline import AnyDepthModel


def test_views_entries_are_declared_exported_and_mirrored(repo_root):
    header = open(os.path.join(repo_root, "include", "mi_depth.h")).read()
    lib = _lib.load()
    for name, nargs in (("md_da3_infer_views", 10), ("md_op_attention_views", 9)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"libmi_depth.so does not export {name}"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
    assert re.search(r"#define\s+MD_OP_POISON_PAD\s+0x200", header) and ops.POISON_PAD == 0x200
    assert callable(ops.attention_views) and callable(DepthAnything3.infer_views) and callable(AnyDepthModel.infer_views)
