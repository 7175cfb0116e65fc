# select.mk (./Makefile's programs + the C++ API tests of the batched sort, reduce and scan, of key runs and of select) plus the
# C++ API test of sorted search (test_sorted_search_api.cpp), through the same variables and pattern rule:
#   make -C tests/cpp -f sorted_search.mk
include select.mk
.DEFAULT_GOAL := with_sorted_search
with_sorted_search: with_select $(BIN)/test_sorted_search_api
.PHONY: with_sorted_search
