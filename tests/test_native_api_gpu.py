"""The native boundary (csrc/sq_api.h + csrc/module.cpp): every binding's
argument format is derived from its launcher's prototype and appended to its
docstring as an ``args:`` line.  ``tests/golden/native_formats.json`` is the
table of those formats as the hand-written wrappers had them (extracted from
their ``PyArg_ParseTuple`` literals, not from the binder), so a prototype
whose types drift from what the Python callers pass fails here.  Needs only
the built extension: nothing is launched."""
import json
import os

import pytest

from sq_learn_amd.ops import _native as nat

pytestmark = pytest.mark.gpu

HAND_WRITTEN = {"xtx_geometry", "device_arch"}

with open(os.path.join(os.path.dirname(__file__), "golden", "native_formats.json")) as f:
    FORMATS = json.load(f)


def _methods():
    m = nat.native()
    return {name: getattr(m, name) for name in dir(m)
            if not name.startswith("_") and callable(getattr(m, name))}


def test_exported_names_match_the_table():
    assert set(_methods()) == set(FORMATS) | HAND_WRITTEN


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_format_matches_the_table(name):
    doc = getattr(nat.native(), name).__doc__
    head, sep, fmt = doc.rpartition("\n\nargs: ")
    assert sep and head, doc
    assert fmt == FORMATS[name]


def test_wrong_argument_count_is_a_type_error():
    m = nat.native()
    with pytest.raises(TypeError):
        m.row_norms(0, 0, 0)
    with pytest.raises(TypeError):
        m.row_norms(0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(TypeError):
        m.spmm_tile_cols(1)


def test_int_slot_overflow_is_an_overflow_error():
    # row_norms: "KiKLiK" - the second slot is an int
    with pytest.raises(OverflowError):
        nat.native().row_norms(0, 1 << 40, 0, 0, 0, 0)


def test_value_binding_returns_its_integer():
    cols = nat.native().spmm_tile_cols()
    assert isinstance(cols, int) and cols > 0
