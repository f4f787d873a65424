"""CLI: ``python -m uncertaintyquantification_sleepapnea_1dcnn_amd.cli.analyze_patient_severity`` (see commands.py)."""
from .commands import analyze_patient_severity

if __name__ == "__main__":
    analyze_patient_severity()
