"""ptss.py says of itself that nothing in it imports torch: callers bring it. A fresh interpreter that imports the binding and loads the
device library must not have torch afterwards."""
import os
import subprocess
import sys

import ptss


def test_the_binding_leaves_torch_unimported():
    code = "import sys, ptss; ptss.device_lib(); ptss.host_lib(); sys.exit(1 if 'torch' in sys.modules else 0)"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.abspath(ptss.__file__)), os.environ.get("PYTHONPATH", "")]))
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr or "torch was imported"
