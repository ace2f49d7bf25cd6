# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_explicit.so = libmpcqp_emu_est.so + the ExplicitMPC launchers (emu_explicit.cpp).
# A makefile of its own: libmpcqp_emu.so and libmpcqp_emu_est.so stay the libraries WITHOUT those launchers.
include Makefile
libmpcqp_emu_explicit.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o
-include emu_explicit.d
