"""What the library's host code decides for a conv -- kernel, halo tile, tiles per work-group, loader and compute
waves, statistics slots, in_norm eligibility, the pair's shared launch -- is case for case what
tests/golden/conv_dispatch_signatures.json records (tools/conv_dispatch_signature.py: one text line per conv and
setting; the file keeps a sha256 and a line count per setting).  The file is the yardstick for a rewrite of the
dispatch: recorded from the library as it stood before the rewrite, never regenerated from the code under test.
Where a setting differs, `python tools/conv_dispatch_signature.py --dump SETTING` on both revisions shows the convs
that moved.  Host arithmetic only: nothing is launched, and without a device the library assumes MI355X's 256 CUs."""
import functools
import importlib.util
import json
import os

import pytest

import conv_forms as CF
from conftest import GOLDEN, REPO

_spec = importlib.util.spec_from_file_location("conv_dispatch_signature",
                                               os.path.join(REPO, "tools", "conv_dispatch_signature.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

with open(os.path.join(GOLDEN, "conv_dispatch_signatures.json")) as _fh:
    RECORDED = json.load(_fh)


@functools.lru_cache(maxsize=None)
def _text(setting):
    return S.text_of(setting)


@pytest.mark.parametrize("setting", S.SETTINGS)
def test_dispatch_matches_recorded_signature(setting):
    assert setting in RECORDED, f"{setting} is not recorded"
    assert S.digest(_text(setting)) == RECORDED[setting], setting


def test_recorded_file_covers_the_settings():
    assert sorted(RECORDED) == sorted(S.SETTINGS) and len(S.SETTINGS) == 15
    # every knob moves at least one case: no two settings share a text
    assert len({v["sha256"] for v in RECORDED.values()}) == len(S.SETTINGS)


def test_default_signature_is_not_vacuous():
    """Every distinct form of conv_forms.TABLE and ENC_TABLE occurs under the default setting, and at least half of
    the random shapes are accepted (return code 0)."""
    lines = _text("default").splitlines()
    assert len(lines) == len(S.cases())
    own = [ln.split(" | ")[0] for ln in lines]   # (without the pair query)
    seen = {ln.split(" form=")[1].split()[0] for ln in own if " rc=0 " in ln}
    want = {",".join(str(v) for v in c.form) for c in CF.TABLE + CF.ENC_TABLE}
    assert want <= seen, sorted(want - seen)
    rand = [ln for ln in lines if ln.startswith("random/")]
    assert len(rand) == S.N_RANDOM
    assert 2 * sum(" rc=0 " in ln.split(" | ")[0] for ln in rand) >= len(rand)
    # the pair query is exercised on both of its routes
    assert any(" one=1 " in ln for ln in lines) and any(" one=0 " in ln for ln in lines)
