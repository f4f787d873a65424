"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_pass_convergence`` (see commands.py)."""
from .commands import analyze_pass_convergence

if __name__ == "__main__":
    analyze_pass_convergence()
