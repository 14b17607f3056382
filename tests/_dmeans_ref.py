"""The reference's q-means estimator functions, AST-extracted verbatim from
``sklearn/cluster/_dmeans.py`` of a checkout of the reference (the module
itself cannot be imported - it needs ``matlab.engine`` and the compiled
Cython extensions).  Extracted: ``labels_estimation`` (:732-777),
``select_labels`` (:2252-2257), ``_centers_update`` (:780-830), ``wrapper``
(:725-727).  They run against the reference's own ``QuantumUtility/
Utility.py`` (``ipe``, ``tomography``) and scikit-learn's ``row_norms``.
Nothing is copied into the framework: the source is read when the recorded
outputs under tests/golden/ and tests/fixtures/ are (re)generated
(tests/golden/make_pinned_ref.py, tests/fixtures/make_dmeans_ref.py); the
checkout's root comes from ``SQ_REFERENCE_ROOT``.  The tests themselves read
only the recorded outputs."""
import ast
import importlib.util
import itertools
import os
import random
import warnings

import numpy as np

FUNCS = ("labels_estimation", "select_labels", "_centers_update", "wrapper")


def _paths():
    root = os.environ.get("SQ_REFERENCE_ROOT", "")
    return (os.path.join(root, "sklearn", "cluster", "_dmeans.py"),
            os.path.join(root, "sklearn", "QuantumUtility", "Utility.py"))


def available():
    return bool(os.environ.get("SQ_REFERENCE_ROOT")) and all(os.path.exists(p) for p in _paths())


def load_utility():
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("_ref_utility_dm", _paths()[1])
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec.loader.exec_module(mod)
    return mod


def load():
    """Namespace with the extracted reference functions."""
    import scipy as sc
    import scipy.spatial  # noqa: F401  (sc.spatial.distance.cdist)
    from sklearn.utils.extmath import row_norms
    U = load_utility()
    DMEANS = _paths()[0]
    tree = ast.parse(open(DMEANS).read())
    keep = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in FUNCS]
    assert {f.name for f in keep} == set(FUNCS), [f.name for f in keep]
    mod = ast.Module(body=keep, type_ignores=[])
    ns = {"np": np, "sc": sc, "random": random, "itertools": itertools, "row_norms": row_norms,
          "ipe": U.ipe, "tomography": U.tomography}
    exec(compile(mod, DMEANS, "exec"), ns)
    return ns, U
