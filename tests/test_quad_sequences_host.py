"""The generator of the CDQuadraticLoss operation sequences (tests/_quad_sequences.py), on the oracle's side alone: every
sequence is 12 to 15 operations of which none is skipped, every operation is drawn, every solve the oracle runs converges
within maxIter (asserted where it runs), and a sequence is a function of its seed."""
import collections

from _quad_sequences import OPS, _run_sequence


def test_the_30_sequences_run_whole_on_the_oracle():
    seen = collections.Counter()
    for seed in range(30):
        ran = _run_sequence(seed, device=False)              # raises where an oracle solve does not converge
        assert 12 <= len(ran) <= 15 and ran == _run_sequence(seed, device=False), seed
        seen.update(ran)
    assert set(seen) == set(OPS) and min(seen.values()) >= 20, seen
