"""Opening a golden fixture: ``np.load`` with ``"x"`` filled in where the file holds the input's seed instead of the array
(tests/golden/synth.py::Fixture: regenerated once per open file, checked against the stored fp64 sum to 1e-6)."""
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

from synth import Fixture as load_npz      # noqa: E402, F401
