"""For the CPU tests that drive a stand-alone host check: load(name) gives the driver tools/<name>_host_check.py as a module, and
needs_compiler skips a test where no host C++ compiler is found."""
import importlib.util
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.append(TOOLS)                     # the drivers import tools/host_check.py by name

import host_check  # noqa: E402


def load(name):
    spec = importlib.util.spec_from_file_location(name + "_host_check", os.path.join(TOOLS, name + "_host_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


needs_compiler = pytest.mark.skipif(host_check.compiler() is None, reason="no host C++ compiler found")
