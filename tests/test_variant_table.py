"""The kernel-selection knobs have ONE table, include/svihmm_debug.h: the SVIHMM_VAR_* enumerators there and
``_lib.VARIANT`` name the same slots, and ``Engine.set_variant`` takes a slot by either."""
import os
import re

import pytest

from pysvihmm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HISTORICAL = ["svi_loop", "stats", "fb", "emission_mt", "pipeline", "emission_orbit", "chain"]


def _header():
    src = open(os.path.join(REPO, "include", "svihmm_debug.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_slot_names_of_the_header_and_the_binding_agree():
    pairs = re.findall(r"\bSVIHMM_VAR_([A-Z0-9_]+)\s*=\s*(\d+)", _header())
    names = [n.lower() for n, _ in pairs]
    assert len(set(names)) == len(names) == 18
    slots = {n.lower(): int(i) for n, i in pairs}
    assert sorted(slots.values()) == list(range(18))
    assert slots == _lib.VARIANT


def test_array_size():
    assert re.findall(r"#define\s+SVIHMM_NVARIANT\s+(\d+)", _header()) == ["24"]


def test_historical_names_keep_their_slots():
    assert [_lib.VARIANT[n] for n in HISTORICAL] == list(range(7))


@pytest.mark.gpu
def test_set_variant_by_name_and_by_index():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    try:
        for name, idx in _lib.VARIANT.items():
            e.set_variant(name, 1)
            e.set_variant(idx, 0)
        for which in (24, -1):
            with pytest.raises(RuntimeError, match=r"^set_variant failed: svihmm_set_variant: bad arguments$"):
                e.set_variant(which, 0)
        with pytest.raises(KeyError):
            e.set_variant("no_such_slot", 0)
        # results would be invalid: only the measurement build knows this code
        with pytest.raises(RuntimeError, match="^" + re.escape(
                "set_variant failed: svihmm_set_variant: measurement-only code (build with -DSVIHMM_MEASURE: "
                "make measure)") + "$"):
            e.set_variant("sweep_family", 9)
    finally:
        for idx in range(18):
            e.set_variant(idx, 0)
        e.close()
