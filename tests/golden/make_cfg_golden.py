#!/usr/bin/env python3
"""Generate tests/golden/cfg_defaults.json: the REFERENCE's default configuration tree (skoots/config.py).

Run where the reference checkout is available (the tests read only the committed .json):

    REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cfg_golden.py

yacs is not needed: ``yacs.config.CfgNode`` is replaced by an attribute dict with ``clone``, and skoots/config.py is
loaded by path so that the package's ``__init__`` and its imports stay out of it.  The file holds settings only.
JSON turns tuples into lists; tests compare modulo that.
"""
import copy
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


class CfgNode(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None

    def __setattr__(self, k, v):
        self[k] = v

    def clone(self):
        return copy.deepcopy(self)


def plain(node):
    if isinstance(node, dict):
        return {k: plain(v) for k, v in node.items()}
    if isinstance(node, (list, tuple)):
        return [plain(v) for v in node]
    return node


def main():
    ref = os.environ.get("REFERENCE") or next((p for p in sys.path if os.path.exists(os.path.join(p, "skoots", "config.py"))), None)
    if ref is None:
        raise SystemExit("set REFERENCE to the reference checkout")
    yacs = types.ModuleType("yacs")
    yacs.config = types.ModuleType("yacs.config")
    yacs.config.CfgNode = CfgNode
    sys.modules["yacs"], sys.modules["yacs.config"] = yacs, yacs.config
    spec = importlib.util.spec_from_file_location("_reference_config", os.path.join(ref, "skoots", "config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    tree = plain(mod.get_cfg_defaults())
    out = os.path.join(HERE, "cfg_defaults.json")
    with open(out, "w") as f:
        json.dump(tree, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes; sections:", sorted(tree))


if __name__ == "__main__":
    main()
