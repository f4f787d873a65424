"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_calibration`` (see commands.py)."""
from .commands import analyze_calibration

if __name__ == "__main__":
    analyze_calibration()
