"""Subprocess body of test_exact_hits_through_a_stack_of_cards: run with DMT_HIP_LIB pointing at a variant build of the HIP
library.  Runs the whole stack case (expected hits from the solid probes and the host twin, brute force and BVH under the
cutout rule) and prints a digest of the results for the caller to compare with the default build's."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from test_cutout_gpu import _stack_case  # noqa: E402

pkg = graft.load_package()
O = graft.load_oracle()
O.build()
with pkg.Renderer(0) as r:
    print(json.dumps({"lib": str(pkg.library_path()), "digest": _stack_case(r, pkg, O)}))
