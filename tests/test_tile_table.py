"""CPU: the mixed-class tile kernel's compact matrix table (x266_tables.hpp: TileTab) and the lane-level image construction the
kernel performs from it, restated in C++ (tests/cpp/tile_table_check.cpp), reproduce the per-class operand images of every
(type, size) class -- built-in matrices and random int8 ones.  g++ only: no GPU, no HIP."""
import _cpp_driver


@_cpp_driver.needs_gxx
def test_tile_table_reproduces_the_per_class_images(tmp_path):
    exe, r = _cpp_driver.build(tmp_path, "tile_table_check")
    assert r.returncode == 0, r.stderr[-2000:]
    _cpp_driver.run(exe, "reproduce the per-class images")
