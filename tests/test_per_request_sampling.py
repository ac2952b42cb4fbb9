"""Per-request sampling settings and seeds through the CPU path of
``inference/continuous.py`` (``sample_ref`` with the tail kernel's noise indexing)."""
import pytest

from dist_utils import run_dist
from test_continuous import CAP
from test_inference import _argv, _setup

PROMPT, OTHERS = [5, 35, 8, 9, 7], ([3, 14, 15], [2, 7, 1, 8, 2, 8], [9, 9])


def _decoder(model, **kw):
    from epfl_megatron_amd.inference import RaggedSamplingDecoder
    from epfl_megatron_amd.inference.forward_step import InferenceParams
    return RaggedSamplingDecoder(model, InferenceParams(2, CAP), 2, 8, vocab_size=250,
                                 capture=False, **kw)


def _cpu_run(rank, world):
    from epfl_megatron_amd.inference import ContinuousBatcher
    model, out = _setup(_argv()), []
    # the seeded request in row 1 beside a greedy one, then third in the queue (row 0)
    seeded = (PROMPT, 7, dict(top_p=0.9, temperature=0.8, seed=4321))
    for requests in ([(OTHERS[0], 5, dict(top_k=1)), seeded],
                     [(OTHERS[1], 3, {}), (OTHERS[2], 6, {}), seeded, (OTHERS[0], 4, dict(top_k=3))]):
        dec = _decoder(model, per_row=True, return_log_probs=True)
        dec.configure(temperature=1.1)
        cb = ContinuousBatcher(model, dec.ip, 2, CAP, poll_every=1, decoder=dec)
        for prompt, mn, kw in requests:
            cb.submit(prompt, mn, **kw)
        out.append((cb.run(), cb.log_probs, cb.primed))
    return out


def test_seeded_request_is_independent_of_its_row_and_neighbours():
    (res_a, lp_a, primed_a), (res_b, lp_b, primed_b) = run_dist(_cpu_run, 1)[0]
    assert len(res_a[1]) == len(lp_a[1]) == 7 and res_a[1] == res_b[2] and lp_a[1] == lp_b[2]
    where = [[p[0] for p in primed if p[1:] == (len(PROMPT), 6)] for primed in (primed_a, primed_b)]
    assert where == [[1], [0]]  # another row, other neighbours
    assert len(set(res_a[1])) > 2  # sampled, not a constant


@pytest.mark.parametrize("sampling,error", [(dict(top_k=5, top_p=0.5), "both top-k and top-p"),
                                            (dict(temperature=0.0, seed=3), "temperature")])
def test_prime_validates_the_row_settings(sampling, error):
    dec = _decoder(None, per_row=True)
    with pytest.raises(AssertionError, match=error):
        dec.prime(0, 1, 4, 3, sampling=sampling)
    dec.prime(0, 1, 4, 3, sampling=dict(top_k=5, temperature=0.5, seed=1))
    assert dec.row_ctl[0].tolist() + dec.row_fctl[0].tolist() == [1, 0, 5, -1, 0.5, 0.0]
