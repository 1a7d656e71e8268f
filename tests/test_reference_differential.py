"""CPU: a short, seeded run of tests/fuzz/fuzz_vs_reference.py -- the oracle's host half (oracle/host_ref.py) and the product's host
functions against the reference's OWN FUNCTIONS on random inputs under the same seeds, exact equality.  The reference's side comes from
tests/golden/reference_differential.json: what its functions returned in the same 40 rounds (seed 77), written by that script's
`record=` mode where the reference can be imported (values, or digests of large arrays), so this test needs nothing outside the
repository.  The long live runs are recorded in profiles/r03/fuzz.txt."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_functions_against_the_imported_reference():
    recorded = os.path.join(HERE, "golden", "reference_differential.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "fuzz", "fuzz_vs_reference.py"), "replay=" + recorded], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "40 rounds against the reference's recorded results: 0 mismatches" in r.stdout
