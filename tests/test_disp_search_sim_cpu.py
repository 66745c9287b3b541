"""The CPU restatement of the fitDisp line search (tools/disp_search_sim.py) on 40 genes of the C3 shape: the evaluator policy
of csrc/fit_disp.hip (likelihood-only at the first proposal and, after a rejection, while kappa > gamma kstar) sends a large
share of the proposals through the likelihood alone and is almost never wrong about them.  Conditions with margin, not
measurements: at 300 genes the first share was 0.3 % or less and the second 42 - 56 % (profiles/disp_predict.md)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def study():
    spec = importlib.util.spec_from_file_location("disp_search_sim", os.path.join(ROOT, "tools", "disp_search_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    return sim.study("C3", genes=40, seed=1, sf_random=True, xs=(0.77,))


@pytest.mark.parametrize("leg", ["gene-wise", "MAP"])
def test_policy_sends_many_proposals_likelihood_only_and_few_of_them_continue(study, leg):
    sent, _, continued = study[leg]["share"][1.0]
    assert continued <= 0.05, "accepted-and-continued among the likelihood-only proposals: %.4f" % continued
    assert sent >= 0.30, "share of the proposals sent likelihood-only: %.4f" % sent
