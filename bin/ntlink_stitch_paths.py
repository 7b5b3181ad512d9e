#!/usr/bin/env python3
"""Drop-in for the reference's `ntlink_stitch_paths.py`, the stitch-paths stage (see ntlink_amd/cli.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.realpath(__file__))))
from ntlink_amd.cli import stitch_paths_main

sys.exit(stitch_paths_main())
