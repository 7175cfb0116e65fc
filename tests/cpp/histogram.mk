# merge.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan, of key runs, of select, of sorted search
# and of merge) plus the C++ API test of histogram (test_histogram_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f histogram.mk
include merge.mk
.DEFAULT_GOAL := with_histogram
with_histogram: with_merge $(BIN)/test_histogram_api
.PHONY: with_histogram
