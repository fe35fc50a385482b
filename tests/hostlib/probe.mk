# Builds tests/_build/probe_print: the counting rules of device/zmx_probe.h as a plain C++ program (probe_print.cc).
# SANITIZE="-fsanitize=address,undefined" OUT_NAME=probe_print_san builds it with sanitizers under another name.
ROOT := $(abspath ../..)
HOST := $(ROOT)/zopfli_amd/csrc/host
DEV  := $(ROOT)/zopfli_amd/csrc/device
OUT  := $(ROOT)/tests/_build
OUT_NAME ?= probe_print

$(OUT)/$(OUT_NAME): probe_print.cc $(DEV)/zmx_probe.h $(HOST)/deal.cc $(HOST)/deal.h
	mkdir -p $(OUT)
	g++ -O1 -std=c++17 -Wall -Wextra -ffp-contract=off $(SANITIZE) -I$(ROOT)/include -I$(HOST) -I$(DEV) -o $@ probe_print.cc $(HOST)/deal.cc
