# histogram.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan, of key runs, of select, of sorted search,
# of merge and of histogram) plus the C++ API test of expand (test_expand_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f expand.mk
include histogram.mk
.DEFAULT_GOAL := with_expand
with_expand: with_histogram $(BIN)/test_expand_api
.PHONY: with_expand
