"""Subprocess body of test_brute_cull_levels_give_the_same_films: run with DMT_BRUTE_CULL in the environment, which a context
reads when it is created.  Runs the route of test_scene_state_gpu._route_digest and prints the digest of its films for the
caller to compare with the default level's."""
import json
import os
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import __graft_entry__ as graft  # noqa: E402
from test_scene_state_gpu import _World, _route_digest  # noqa: E402

pkg = graft.load_package()
with tempfile.TemporaryDirectory() as tmp:
    print(json.dumps({"level": os.environ.get("DMT_BRUTE_CULL"), "digest": _route_digest(pkg, _World(pkg, Path(tmp)))}))
