# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_sim.so = libmpcqp_emu_est.so + the ExplicitMPC launchers (emu_explicit.cpp) + the
# plant of the closed-loop simulation (emu_sim.cpp).  A makefile of its own: the other libraries stay WITHOUT that launcher.
include Makefile
libmpcqp_emu_sim.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o
-include emu_explicit.d emu_sim.d
