"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_laplace_patient_level`` (see commands.py)."""
from .commands import analyze_laplace_patient_level
from ..uq.drivers import evaluate_laplace  # noqa: F401

if __name__ == "__main__":
    analyze_laplace_patient_level()
