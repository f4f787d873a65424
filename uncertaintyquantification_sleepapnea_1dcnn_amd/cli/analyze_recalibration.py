"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_recalibration`` (see commands.py)."""
from .commands import analyze_recalibration

if __name__ == "__main__":
    analyze_recalibration()
