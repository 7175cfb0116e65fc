# sorted_search.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan, of key runs, of select and of
# sorted search) plus the C++ API test of merge (test_merge_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f merge.mk
include sorted_search.mk
.DEFAULT_GOAL := with_merge
with_merge: with_sorted_search $(BIN)/test_merge_api
.PHONY: with_merge
