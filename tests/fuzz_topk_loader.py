"""Loads tools/fuzz_topk.py as a module (test infrastructure), for the GPU run of it and for the CPU test of its generator."""
import importlib.util
import os


def load_fuzz():
    spec = importlib.util.spec_from_file_location("fuzz_topk", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_topk.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz
