"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_ensemble_members`` (see commands.py)."""
from .commands import analyze_ensemble_members

if __name__ == "__main__":
    analyze_ensemble_members()
