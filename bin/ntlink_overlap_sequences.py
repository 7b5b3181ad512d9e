#!/usr/bin/env python3
"""Drop-in for the reference's `ntlink_overlap_sequences.py`, the overlap-trimming stage (see ntlink_amd/cli.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from ntlink_amd.cli import overlap_sequences_main

sys.exit(overlap_sequences_main())
