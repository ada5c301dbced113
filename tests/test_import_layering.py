"""The import graph of the network modules is strictly downward (CPU, no compute):

    _lib <- fused <- dense <- { na, nat, swin, vit, heads, gennet } <- segnet <- { ppnet, train }        configs: imports nothing

Every import of a sibling in dense / nat / heads / configs / swin / vit / segnet is at module level (none hidden inside a function),
nothing below segnet names segnet, and importing a backbone or the heads does not load segnet."""
import ast
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ppnet_amd")
TOP_LEVEL_ONLY = ("dense", "nat", "heads", "configs", "swin", "vit", "segnet")
BELOW_SEGNET = ("dense", "nat", "heads", "configs", "swin", "vit", "na", "gennet", "fused")


def _sibling_imports(module):
    """[(line, names of the siblings imported, at module level?)] for every relative import of ppnet_amd/<module>.py."""
    tree = ast.parse(open(os.path.join(PKG, module + ".py")).read())
    top = {id(n) for n in tree.body}
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level > 0:
            names = [node.module.split(".")[0]] if node.module else [a.name for a in node.names]
            out.append((node.lineno, names, id(node) in top))
    return out


def test_network_modules_import_strictly_downward():
    hidden = [f"{m}.py:{line}" for m in TOP_LEVEL_ONLY for line, _, at_top in _sibling_imports(m) if not at_top]
    assert not hidden, f"sibling imports inside functions: {hidden}"
    upward = [f"{m}.py:{line}" for m in BELOW_SEGNET for line, names, _ in _sibling_imports(m) if "segnet" in names]
    assert not upward, f"modules below segnet import it: {upward}"
    assert _sibling_imports("configs") == []
    # and at run time, in a fresh interpreter
    code = ("import sys, ppnet_amd.swin, ppnet_amd.vit, ppnet_amd.nat, ppnet_amd.heads; "
            "assert 'ppnet_amd.segnet' not in sys.modules, 'a backbone or the heads pulled in ppnet_amd.segnet'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
