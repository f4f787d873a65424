"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_shift_robustness`` (see commands.py)."""
from .commands import analyze_shift_robustness

if __name__ == "__main__":
    analyze_shift_robustness()
