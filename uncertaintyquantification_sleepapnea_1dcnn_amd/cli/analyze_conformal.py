"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_conformal`` (see commands.py)."""
from .commands import analyze_conformal

if __name__ == "__main__":
    analyze_conformal()
