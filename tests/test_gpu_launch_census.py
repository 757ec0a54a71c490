"""The launches of an encode and a decode call are the recorded ones (-m gpu): tests/golden/launch_census.json holds, per case of
tests/golden/make_launch_census.py, the launch count of every timing kind after each of the two calls, the form of the last
k_search_long launch and the count of exact fallbacks, as recorded on the MI355X.  A change of the host's launch code that is meant
to leave the launches alone must reproduce every count.  Output values are not compared here: the parity tests do that.

What a count cannot show: a timing kind is one span per launch site, so two cases record what the case without their knob records
and are NOT coverage of the forms they name.  m7_f1_lev_wave0: kind 4 is one span per layer whether Levinson-Durbin runs as one
k_levinson_wave launch or as several k_levinson_lds launches.  m7_f40_hist_fwdloss_lastlayer2: the 777-sample tail is not
k_fwd_loss's, which keeps k_last_layer off for the chunk whatever LINNE_AMD_LAST_LAYER says.  tests/test_forms_cpu.py checks both
rules; the cases stay because the knobs must at least leave every other launch alone."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_launch_census", os.path.join(HERE, "golden", "make_launch_census.py"))
census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(census)


@pytest.fixture(scope="module")
def golden():
    with open(census.OUT) as fh:
        return json.load(fh)


def test_every_case_is_recorded(golden):
    assert sorted(golden) == sorted(census.CASE_NAMES)


@pytest.mark.parametrize("case", census.CASES, ids=census.CASE_NAMES)
def test_launches_are_the_recorded_ones(case, golden, monkeypatch):
    for v in list(os.environ):
        if v.startswith("LINNE_AMD_") and v != "LINNE_AMD_LIB":
            monkeypatch.delenv(v)
    got = census.run_case(case, monkeypatch.setenv)
    want = golden[case["name"]]
    print(case["name"], got)
    for call in ("encode", "decode"):
        for kind in census.KINDS:
            assert got[call].get(str(kind), 0) == want[call].get(str(kind), 0), \
                f"{call}: kind {kind}: {got[call].get(str(kind), 0)} launches, {want[call].get(str(kind), 0)} recorded ({got[call]} against {want[call]})"
    assert got["search_long_form"] == want["search_long_form"]
    assert got["fallbacks"] == want["fallbacks"]
