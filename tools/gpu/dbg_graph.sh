python tools/gpu/dbg_graph.py default 2>&1 | tail -8
