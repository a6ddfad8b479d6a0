"""Record tests/golden/boundary.json: the reference side of tests/test_boundary_conformance.py -- parameter names and
defaults of the reference's operator wrappers (parsed with `ast` from its Python sources, with regular expressions from its
Cython files), the arity of its pybind entry points (C++ declarations), and the native-operator imports
(`from mmdet.ops... import ...`) of the reference Python files the test names.  Run where the reference tree is
(python tests/golden/make_golden_boundary.py <reference root>); the fixture is committed."""
import ast
import importlib.util
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def encode(v):
    if isinstance(v, tuple):
        return {"__tuple__": [encode(x) for x in v]}
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


def sig_from_ast(fn, drop_first=0):
    """[(name, default or None)] of an ast.FunctionDef (positional + keyword parameters)."""
    args = fn.args.args[drop_first:]
    defaults = [None] * (len(fn.args.args) - len(fn.args.defaults)) + list(fn.args.defaults)
    defaults = defaults[drop_first:]
    out = []
    for a, d in zip(args, defaults):
        out.append((a.arg, None if d is None else ast.literal_eval(d)))
    if fn.args.vararg:
        out.append(('*' + fn.args.vararg.arg, None))
    if fn.args.kwarg:
        out.append(('**' + fn.args.kwarg.arg, None))
    return out


def find(tree, name, cls=None):
    body = tree.body
    if cls is not None:
        body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0].body
    return [n for n in body if isinstance(n, ast.FunctionDef) and n.name == name][0]


def pyx_params(src, fname):
    m = re.search(r"def\s+%s\s*\((.*?)\):" % fname, src, re.S)
    params = re.sub(r"\[[^\]]*\]", "", m.group(1))            # drop the Cython buffer declarations [dtype, ndim=2]
    out = []
    for part in params.split(","):
        part = part.strip()
        if "=" in part:
            left, d = part.split("=")
            out.append((left.split()[-1], ast.literal_eval(d.strip())))
        else:
            out.append((part.split()[-1], None))
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ORP_REFERENCE_ROOT")
    if not ref:
        raise SystemExit("usage: make_golden_boundary.py <reference root> (or ORP_REFERENCE_ROOT)")
    spec = importlib.util.spec_from_file_location("test_boundary_conformance", os.path.join(ROOT, "tests", "test_boundary_conformance.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)

    def read(rel):
        with open(os.path.join(ref, rel)) as f:
            return f.read()
    out = {"signatures": {}, "pyx": {}, "pybind_arity": {}, "operator_imports": []}
    for key, rel, fn, cls, drop in t.SIGNATURES:
        out["signatures"][key] = [[n, encode(d)] for n, d in sig_from_ast(find(ast.parse(read(rel)), fn, cls), drop)]
    for key, rel, fn in t.PYX:
        out["pyx"][key] = [[n, encode(d)] for n, d in pyx_params(read(rel), fn)]
    for key, rel, pattern in t.PYBIND:
        out["pybind_arity"][key] = len(re.search(pattern, read(rel), re.S).group(1).split(","))
    for rel in t.IMPORTING_FILES:
        for node in ast.walk(ast.parse(read(rel))):
            if isinstance(node, ast.ImportFrom) and node.level == 0 and (node.module or "").startswith("mmdet.ops"):
                out["operator_imports"] += [[rel, node.module, a.name] for a in node.names]
    with open(os.path.join(HERE, "boundary.json"), "w") as g:
        json.dump(out, g, indent=1)
        g.write("\n")


if __name__ == "__main__":
    main()
