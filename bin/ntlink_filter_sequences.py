#!/usr/bin/env python3
"""Drop-in for the reference's `ntlink_filter_sequences.py`, the filter in front of the overlap sketch (see ntlink_amd/cli.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from ntlink_amd.cli import filter_sequences_main

sys.exit(filter_sequences_main())
