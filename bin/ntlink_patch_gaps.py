#!/usr/bin/env python3
"""Drop-in for the reference's `ntlink_patch_gaps.py`, the gap-filling stage (see ntlink_amd/cli.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from ntlink_amd.cli import patch_gaps_main

sys.exit(patch_gaps_main())
