"""Writer of the measured-figures records under profiles/ (profiles/r10/device_math_errors.json): with PK_FIGURES_JSON naming a
file, every record() call of the GPU tests merges its figures into that JSON, beside the revision of the library (git, or
PK_FIGURES_REVISION where the tree travels without its history), the host and the card.  Without the variable: nothing."""
import json
import os
import platform
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _revision():
    if os.environ.get("PK_FIGURES_REVISION"):
        return os.environ["PK_FIGURES_REVISION"]
    try:
        rev = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.call(["git", "diff", "--quiet", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL) != 0
        return rev + ("+uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def _card():
    try:
        import torch

        name = torch.cuda.get_device_name(0)
        return "%s (%s)" % (name, getattr(torch.cuda.get_device_properties(0), "gcnArchName", "architecture not reported"))
    except Exception:
        return os.environ.get("PK_FIGURES_CARD", "unknown")


def record(section, name, _what=None, **figures):
    """_what: what a record of its own says of itself (profiles/r10/ekf_errors.json), where it is not the one above"""
    path = os.environ.get("PK_FIGURES_JSON")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault("what", _what or "worst errors of the float64 device primitives against mpmath / numpy.longdouble "
                           "(tests/test_gpu_math_probe.py) and the resampler / pose sums at large particle counts "
                           "(tests/test_gpu_particle_edges.py), written by the tests: PK_FIGURES_JSON=<this file> pytest -m gpu <both>")
    doc["library_revision"], doc["host"], doc["card"] = _revision(), platform.node(), _card()
    doc.setdefault(section, {}).setdefault(name, {}).update({k: (v if isinstance(v, (int, float, str, bool, list)) else float(v))
                                                             for k, v in figures.items()})
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
