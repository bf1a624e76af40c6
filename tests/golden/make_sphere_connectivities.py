"""Build-container-only script: extracts the NUMBERS of the reference's two remaining cubed-sphere connectivities into JSON fixtures
(data, not source text).

  cubed_sphere_13tree_connectivity.json  p8est_connectivity_new_sphere of p4est 2.8 (third_party/p4est-2.8.tar.gz,
                                         src/p8est_connectivity.c): six outer wedges, six inner wedges, the centre cube; what
                                         [geometry] name = cubed_sphere builds its forest on
                                         (src/Geometry/d4est_geometry_cubed_sphere.c:2070-2100).
  sphere_with_hole_connectivity.json     d4est_connectivity_new_sphere_with_hole
                                         (src/Geometry/d4est_connectivity_cubed_sphere.c:109-181): the same twelve wedges without the
                                         cube, for cubed_sphere_with_sphere_hole and cubed_sphere_with_cube_hole.

Each holds vertices, tree_to_vertex, tree_to_tree and tree_to_face, read out of the initialisers as integer / decimal literals with
a regular expression: nothing of the text is evaluated.

Run from the repo root:  python tests/golden/make_sphere_connectivities.py <reference checkout>   (the fixtures are committed).
"""
import json
import os
import re
import sys
import tarfile

HERE = os.path.dirname(os.path.abspath(__file__))
_NUMBER = r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?"


def literals(text, name, kind):
    """the numeric literals of the initialiser `name[...] = { ... };` inside `text`, comments stripped, in order"""
    m = re.search(r"\b" + re.escape(name) + r"\s*\[[^\]]*\]\s*=\s*\{(.*?)\}\s*;", text, flags=re.S)
    if not m:
        raise ValueError("initialiser %s not found" % name)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    if not re.fullmatch(r"[0-9eE+\-.,\s]*", body):
        raise ValueError("initialiser %s holds more than numeric literals" % name)
    return [kind(v) for v in re.findall(_NUMBER, body)]


def function_text(src, name, end=None):
    """the text of `src` from the DEFINITION of function `name` (its name followed by `(void)`) up to `end` or the next `return`"""
    m = re.search(r"\b" + re.escape(name) + r"\s*\(\s*void\s*\)\s*\{", src)
    if not m:
        raise ValueError("function %s not found" % name)
    stop = src.index(end, m.end()) if end else src.index("return", m.end())
    return src[m.start():stop]


def connectivity(fn, num_trees, source):
    vertices = literals(fn, "vertices", float)
    ttv = literals(fn, "tree_to_vertex", int)
    ttt = literals(fn, "tree_to_tree", int)
    ttf = literals(fn, "tree_to_face", int)
    assert len(vertices) % 3 == 0 and len(ttv) == 8 * num_trees and len(ttt) == 6 * num_trees and len(ttf) == 6 * num_trees, \
        (len(vertices), len(ttv), len(ttt), len(ttf))
    assert max(ttv) < len(vertices) // 3 and max(ttt) < num_trees and max(ttf) < 24
    return {"source": source, "num_trees": num_trees, "vertices": vertices, "tree_to_vertex": ttv, "tree_to_tree": ttt, "tree_to_face": ttf}


def main(ref):
    with tarfile.open(os.path.join(ref, "third_party", "p4est-2.8.tar.gz")) as tf:
        member = [m for m in tf.getmembers() if m.name.endswith("/src/p8est_connectivity.c")][0]
        p8 = tf.extractfile(member).read().decode()
    sphere = connectivity(function_text(p8, "p8est_connectivity_new_sphere"), 13,
                          "third_party/p4est-2.8.tar.gz: src/p8est_connectivity.c, p8est_connectivity_new_sphere (numbers only)")
    csrc = open(os.path.join(ref, "src", "Geometry", "d4est_connectivity_cubed_sphere.c")).read()
    hole = connectivity(function_text(csrc, "d4est_connectivity_new_sphere_with_hole"), 12,
                        "src/Geometry/d4est_connectivity_cubed_sphere.c:109-181, d4est_connectivity_new_sphere_with_hole (numbers only)")
    for name, d in (("cubed_sphere_13tree_connectivity.json", sphere), ("sphere_with_hole_connectivity.json", hole)):
        with open(os.path.join(HERE, name), "w") as fh:
            json.dump(d, fh)
        print("wrote", name)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
