"""The order tables in device memory (g_order_tables, what the camera kernels read) against the
host's and against the kill sets.  Run as a program with ORT_LIB naming the analysis library
(tests/test_gpu_child_order.py): the export hook lives there, and a GPU process must not load it
beside libort.so."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main():
    import octreeraytracer_amd as ort
    from test_child_order import TABLE, order_tables, table_entry
    with ort.Renderer(0):  # (a context: the device is chosen and the library's code object loaded)
        dev = order_tables(device=True)
    host = order_tables()
    want = [table_entry(t, i) for t in (0, 1) for i in range(TABLE)]
    ok = True
    for t in (0, 1):
        same = dev[TABLE * t:TABLE * (t + 1)] == host[TABLE * t:TABLE * (t + 1)] == want[TABLE * t:TABLE * (t + 1)]
        ok = ok and same
        print(f"table {t}: {'equal' if same else 'DIFFERENT'}")
    print(f"all equal: {ok}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
