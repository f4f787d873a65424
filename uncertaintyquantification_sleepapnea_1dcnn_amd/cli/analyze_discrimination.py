"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_discrimination`` (see commands.py)."""
from .commands import analyze_discrimination

if __name__ == "__main__":
    analyze_discrimination()
